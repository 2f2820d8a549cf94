"""CPU restatement of the reference's default training targets: SamplerValues::prepare_training_data (src/dataset/Sampler.cpp:138-214) and
the per-cell weight of the action-value loss (fill_action_values_mask, src/selfplay/SupervisedLearning.cpp:55-61), built like
tests/training_batch_ref.py only from what the oracle exports: ago_sample_v201_unpack (parse + SearchDataStorage_v201::storeTo: prior and
minimax value included), ago_apply_symmetry, ago_encode_features and ago_score_info (proven, distance, value).

values_targets() is Sampler.cpp:148-213 one operation after the other on numpy scalars of ONE dtype: with numpy.float32 it is the yardstick
of the device path (np.log / np.exp on float32), with numpy.float64 the yardstick of the float32 arithmetic itself.  The deliberate
difference from the reference is the device path's own: the sample is transformed first, so every sequential sum runs in cell order of the
TRANSFORMED board (the reference samples first and applies the symmetry afterwards).

The weights follow one rule in every policy mode: c = max(1, visits) on an empty cell with a proven score, visits elsewhere — the count both
samplers leave in TrainingDataPack::visit_count —, w = float32(c) * (1.0f / float32(sum of c)), all 0.0f when the sum is 0.
"""
import ctypes

import numpy as np

import oracle_lib as ol
import training_batch_ref as ref

F32 = np.float32
_info_cache = {}


def score_info(olib, raw):
    """(is proven, proven value 0 loss / 1 draw / 2 unknown / 3 win, distance, win, draw) of a Score's raw bits"""
    raw = int(raw)
    if raw not in _info_cache:
        dist, val = ctypes.c_int(), (ctypes.c_float * 2)()
        flags = olib.ago_score_info(ctypes.c_uint16(raw), ctypes.byref(dist), val)
        _info_cache[raw] = (bool(flags & 1), (raw >> 13) & 3, int(dist.value), F32(val[0]), F32(val[1]))
    return _info_cache[raw]


def unpack(olib, sample, n):
    """storeTo: visits i32[hw], prior f32[hw], value f32[hw, 2], score u16[hw], header (minimax score, move number, flags), minimax value f32[2]"""
    hw = n * n
    visits, prior, value, score = np.zeros(hw, np.int32), np.zeros(hw, np.float32), np.zeros((hw, 2), np.float32), np.zeros(hw, np.uint16)
    header, mm = np.zeros(3, np.int32), np.zeros(2, np.float32)
    sample = np.ascontiguousarray(sample, dtype=np.uint8)
    used = olib.ago_sample_v201_unpack(ol.ptr(sample), n, n, ol.ptr(visits), ol.ptr(prior), ol.ptr(value), ol.ptr(score), ol.ptr(header), ol.ptr(mm))
    assert used == sample.size
    return visits, prior, value, score, header, mm


def fixed_up_counts(board, visits, proven):
    """TrainingDataPack::visit_count as both samplers leave it (Sampler.cpp:112,161)"""
    return np.array([max(1, int(v)) if (b == 0 and p) else int(v) for b, v, p in zip(board, visits, proven)], np.int64)


def weights_of(counts):
    """fill_action_values_mask in float32: count * (1 / sum); all zero when the sum is (the project's rule)"""
    total = int(counts.sum())
    if total == 0:
        return np.zeros(counts.size, np.float32)
    inv = F32(1.0) / F32(total)
    return np.array([F32(int(c)) * inv for c in counts], np.float32)


def values_targets(T, board, visits, prior, win, draw, infos, minimax_value, minimax_info):
    """Sampler.cpp:148-213 in dtype T (numpy.float32 or numpy.float64) on the dequantised sample.  infos: score_info() per cell.  Returns
    (policy T[hw], action values T[hw, 3], stats): the stats are what the tests' non-vacuity conditions look at."""
    hw = board.size
    zero, half, one = T(0.0), T(0.5), T(1.0)
    eps = T(np.finfo(np.float32).eps)            # log_eps is instantiated for float in either case: FLT_EPSILON
    expectation = lambda w, d: T(w) + half * T(d)  # noqa: E731  Value::getExpectation
    empty = [int(board[i]) == 0 for i in range(hw)]
    counted = [empty[i] and (int(visits[i]) > 0 or infos[i][0]) for i in range(hw)]
    av = np.zeros((hw, 3), T)
    av[:, 2] = one - (zero + zero)               # the cleared pack
    sum_PxQ, sum_P, unvisited = zero, zero, 0
    for i in range(hw):
        if not empty[i]:
            continue
        if counted[i]:
            proven, _, _, pw, pd = infos[i]
            w, d = (T(pw), T(pd)) if proven else (T(win[i]), T(draw[i]))   # get_value(action_value, score)
            sum_PxQ = T(sum_PxQ + T(T(prior[i]) * expectation(w, d)))
            sum_P = T(sum_P + T(prior[i]))
            av[i] = (w, d, T(one - T(w + d)))
        else:
            unvisited += 1
    proven, _, _, pw, pd = minimax_info
    V = expectation(pw, pd) if proven else expectation(minimax_value[0], minimax_value[1])
    base = T(T(sum_P * sum_PxQ) + T(T(one - sum_P) * V))
    default_P = zero
    if unvisited > 0:
        spread = T(T(one - sum_P) / T(unvisited))
        default_P = spread if zero < spread else zero     # std::max(0.0f, ...)
    logit = np.zeros(hw, T)
    max_value = None
    for i in range(hw):
        if not empty[i]:
            continue
        Q, P = base, default_P
        if counted[i]:
            _, pv, dist, _, _ = infos[i]
            if pv == 0:
                Q = T(T(-1.0) / T(one + T(dist)))
            elif pv == 1:
                Q = half
            elif pv == 3:
                Q = T(one + T(T(2.0) / T(one + T(dist))))
            else:
                Q = expectation(win[i], draw[i])
            P = T(prior[i])
        logit[i] = T(T(T(50.0) * Q) + np.log(T(eps + P)))
        max_value = logit[i] if max_value is None or logit[i] > max_value else max_value
    policy = np.zeros(hw, T)
    sum_policy, clamped, unclamped = zero, 0, 0
    for i in range(hw):
        if not empty[i]:
            continue
        shifted = T(logit[i] - max_value)
        clamped += int(not (T(-20.0) < shifted))
        unclamped += int(T(-20.0) < shifted)
        policy[i] = np.exp(shifted if T(-20.0) < shifted else T(-20.0))
        sum_policy = T(sum_policy + policy[i])
    for i in range(hw):
        if empty[i]:
            policy[i] = T(policy[i] / sum_policy)
    stats = dict(sum_P=float(sum_P), unvisited=unvisited, clamped=clamped, unclamped=unclamped,
                 wins_without_visits=sum(1 for i in range(hw) if counted[i] and infos[i][1] == 3 and int(visits[i]) == 0),
                 losses=sum(1 for i in range(hw) if counted[i] and infos[i][1] == 0), draws=sum(1 for i in range(hw) if counted[i] and infos[i][1] == 1),
                 visited_unknown=sum(1 for i in range(hw) if counted[i] and infos[i][1] == 2),
                 empty_without_entry=sum(1 for i in range(hw) if empty[i] and not counted[i]))
    return policy, av, stats


def dequantised(olib, n, game, index, augmentation):
    """the sample under the symmetry: visits, prior, win, draw, score, header, minimax value"""
    visits, prior, value, score, header, mm = unpack(olib, game["samples"][index], n)
    s = augmentation
    return (ref.symmetric(olib, n, s, visits), ref.symmetric(olib, n, s, prior), ref.symmetric(olib, n, s, np.ascontiguousarray(value[:, 0])),
            ref.symmetric(olib, n, s, np.ascontiguousarray(value[:, 1])), ref.symmetric(olib, n, s, score), header, mm)


def reference_sample(olib, rules, n, game, index, augmentation, policy="values", dtype=np.float32):
    """one sample -> the dict of training_batch_ref.reference_sample plus `weight` f32[hw] and `stats`; with policy="values" its policy and
    action values are SamplerValues' (in `dtype`), otherwise the visit-count targets of training_batch_ref"""
    base = ref.reference_sample(olib, rules, n, game, index, augmentation, policy if policy != "values" else "torch_api")
    visits, prior, win, draw, score, header, mm = dequantised(olib, n, game, index, augmentation)
    infos = [score_info(olib, x) for x in score]
    counts = fixed_up_counts(base["board"], visits, [i[0] for i in infos])
    base["weight"] = weights_of(counts)
    base["stats"] = dict(weight_sum=int(counts.sum()), sum_visits=int(visits.sum()), minimax_proven=score_info(olib, int(header[0]) & 0xFFFF)[0])
    if policy == "values":
        pol, av, stats = values_targets(dtype, base["board"], visits, prior, win, draw, infos, mm, score_info(olib, int(header[0]) & 0xFFFF))
        base["policy"], base["action_values"] = pol, av
        base["stats"].update(stats)
    return base


def reference_batch(olib, rules, n, fragments, samples, policy="values", dtype=np.float32):
    """fragments: {index: [parsed games]}; samples: rows of (fragment, game, sample, augmentation).  training_batch_ref.reference_batch's
    dict plus action_values_weight [n, rows, cols] and the per-sample stats"""
    rows = [reference_sample(olib, rules, n, fragments[int(f)][int(g)], int(k), int(a), policy) for f, g, k, a in samples]
    feats = np.stack([r["features"] for r in rows])
    return dict(features=feats, input=ref.input_planes(feats, dtype).reshape(len(rows), n, n, 32),
                policy_target=np.stack([r["policy"] for r in rows]).reshape(len(rows), n, n),
                value_target=np.stack([r["value"] for r in rows]), moves_left_target=np.stack([r["moves_left"] for r in rows]),
                action_values_target=np.stack([r["action_values"] for r in rows]).reshape(len(rows), n, n, 3),
                action_values_weight=np.stack([r["weight"] for r in rows]).reshape(len(rows), n, n), stats=[r["stats"] for r in rows])


WIN_IN, LOSS_IN, DRAW_IN, UNKNOWN = (lambda k: (3 << 13) | (4000 - k)), (lambda k: (0 << 13) | (4000 + k)), (lambda k: (1 << 13) | (4000 + k)), \
    (lambda e: (2 << 13) | (4000 + e))


def crafted_games(olib, n):
    """Two hand-made games with what self-play does not reliably supply, non-uniform priors throughout.
    Game 0 (the stones of training_batch_ref.crafted_game):
      sample 0  a proven win WITHOUT visits, a proven loss, a proven draw, a visited unknown edge, every other empty cell without an entry;
                the win against the loss puts the -20 clamp to work
      sample 1  proven edges only, no visits at all: storeTo takes the minimax value from the (proven) minimax score
      sample 2  two visited edges whose priors sum to more than 1: the max(0, ...) clamp of the default P
      sample 3  no entry at all under a proven minimax score: every weight is 0, the policy is uniform
    Game 1: a board with three empty cells left, all three visited: unvisited_actions_count == 0."""
    moves = np.array([ref.move(1, 7, 5), ref.move(2, n - 1, 0), ref.move(1, 7, 6), ref.move(2, n - 1, 2), ref.move(1, 5, 7), ref.move(2, n - 1, 4), ref.move(1, 6, 7),
                      ref.move(2, n - 1, 6), ref.move(1, 0, 0)], np.uint16)
    first = [
        ref.pack_sample(olib, n, 8, [n + 2, n + 5, 2 * n + 1, 2 * n + 6, 3 * n + 3], [0, 5, 0, 37, 2],
                        [[0.9, 0.05], [0.1, 0.2], [0.3, 0.6], [0.45, 0.25], [0.2, 0.1]], [WIN_IN(3), LOSS_IN(2), DRAW_IN(5), UNKNOWN(100), UNKNOWN(-40)],
                        prior=[0.4, 0.1, 0.05, 0.3, 0.02], root_score=WIN_IN(4)),
        ref.pack_sample(olib, n, 4, [n + 3, n + 4], [0, 0], [[0.0, 0.0], [1.0, 0.0]], [LOSS_IN(4), WIN_IN(1)], prior=[0.25, 0.5], root_score=WIN_IN(2)),
        ref.pack_sample(olib, n, 7, [3, 2 * n + 2], [12, 3], [[0.5, 0.1], [0.2, 0.7]], [UNKNOWN(0), UNKNOWN(-250)], prior=[0.7, 0.6]),
        ref.pack_sample(olib, n, 6, [], [], np.zeros((0, 2)), [], prior=[], root_score=DRAW_IN(3)),
    ]
    # XXOO rows, shifted by two from row to row: no line of three anywhere, whatever the rules
    left = [n + 1, 3 * n + 4, 5 * n + 2]
    cells = [c for c in range(n * n) if c not in left]
    full = [ref.move(1 + ((((c % n) // 2) + (c // n)) % 2), c // n, c % n) for c in cells] + [ref.move(1, left[0] // n, left[0] % n)]
    second = [ref.pack_sample(olib, n, len(cells), left, [9, 4, 1], [[0.5, 0.1], [0.3, 0.3], [0.1, 0.2]], [UNKNOWN(10), UNKNOWN(-20), UNKNOWN(0)], prior=[0.5, 0.3, 0.1])]
    return [ref.build_game(first, moves, 2, n), ref.build_game(second, np.array(full, np.uint16), 1, n)]
