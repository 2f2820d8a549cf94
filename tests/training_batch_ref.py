"""CPU restatement of the reference's training-batch loader (src/dataset/torch_api.cpp:185-279, load_batch), built only from what the
oracle exports: ago_sample_v201_unpack (parse + SearchDataStorage_v201::storeTo), ago_apply_symmetry, ago_encode_features
(PatternCalculator::setBoard + NNInputFeatures::encode) and ago_score_info (Score::isProven / convertToValue).

Per sample: board from the game's first move_number moves (GameDataStorage::getSample), sign to move = the sign of move
move_number, the sample dequantised, symmetry `augmentation` applied to the board and to every per-cell array, features encoded on
the transformed board, then the targets of torch_api.cpp:228-272.  The policy sum is a numpy.float32 sum in cell order, one addend
after the other.  Two deliberate differences from torch_api.cpp, the same as the device path's: every sample's action values go to
the sample's own index (the reference never advances that pointer), and policy="visits" gives SamplerVisits' policy target
(Sampler.cpp:117-130: a proven draw keeps its visit count).

torch_api.cpp itself cannot be compiled without MinML, so this restatement is not pinned against a compiled reference.
"""
import ctypes

import numpy as np

import oracle_lib as ol

F32 = np.float32
UNKNOWN_SCORE = (2 << 13) | 4000


def parse_game(data):
    """GameDataStorage::serialize (format 201) bytes -> dict(samples=[bytes of every sample], moves=u16[], outcome, rows, cols)"""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    n_samples = int(data[0:4].view(np.uint32)[0])
    off, samples = 4, []
    for _ in range(n_samples):
        count = int(data[off + 12:off + 16].view(np.uint32)[0])
        samples.append(data[off:off + 16 + 6 * count].copy())
        off += 16 + 6 * count
    n_moves = int(data[off:off + 4].view(np.uint32)[0])
    moves = data[off + 4:off + 4 + 2 * n_moves].view(np.uint16).copy()
    off += 4 + 2 * n_moves
    outcome, rows, cols = (int(x) for x in data[off:off + 12].view(np.int32))
    assert off + 12 == data.size
    return dict(samples=samples, moves=moves, outcome=outcome, rows=rows, cols=cols)


def build_game(samples, moves, outcome, n):
    """the inverse: format-201 game bytes from sample byte strings, u16 moves and an outcome"""
    parts = [np.array([len(samples)], np.uint32).view(np.uint8)] + [np.ascontiguousarray(s, dtype=np.uint8) for s in samples]
    parts += [np.array([len(moves)], np.uint32).view(np.uint8), np.ascontiguousarray(moves, dtype=np.uint16).view(np.uint8),
              np.array([outcome, n, n], np.int32).view(np.uint8)]
    return np.concatenate(parts)


def write_fragment(path, rules_name, n, games, draw_after=None):
    """GameDataBuffer::save's uncompressed layout: one JSON header line, then the games' bytes"""
    offsets, at = [], 0
    for g in games:
        offsets.append(at)
        at += len(g)
    header = '{"format": 201, "config": {"rules": "%s", "rows": %d, "cols": %d, "draw_after": %d}, "offsets": [%s]}\n' % (
        rules_name, n, n, draw_after or n * n, ", ".join(str(o) for o in offsets))
    with open(path, "wb") as f:
        f.write(header.encode())
        for g in games:
            f.write(np.ascontiguousarray(g, dtype=np.uint8).tobytes())


_score_cache = {}


def score_info(olib, raw):
    """(is proven, win, draw) of a Score's raw bits"""
    raw = int(raw)
    if raw not in _score_cache:
        dist, val = ctypes.c_int(), (ctypes.c_float * 2)()
        flags = olib.ago_score_info(ctypes.c_uint16(raw), ctypes.byref(dist), val)
        _score_cache[raw] = (bool(flags & 1), F32(val[0]), F32(val[1]))
    return _score_cache[raw]


def unpack(olib, sample, n):
    hw = n * n
    visits, prior, value, score = np.zeros(hw, np.int32), np.zeros(hw, np.float32), np.zeros((hw, 2), np.float32), np.zeros(hw, np.uint16)
    header, mm = np.zeros(3, np.int32), np.zeros(2, np.float32)
    sample = np.ascontiguousarray(sample, dtype=np.uint8)
    used = olib.ago_sample_v201_unpack(ol.ptr(sample), n, n, ol.ptr(visits), ol.ptr(prior), ol.ptr(value), ol.ptr(score), ol.ptr(header), ol.ptr(mm))
    assert used == sample.size
    return visits, prior, value, score, header


def symmetric(olib, n, s, cells):
    """apply_symmetry_in_place on a per-cell array of 4-byte (or narrower integer) elements"""
    a = np.ascontiguousarray(cells)
    if a.dtype.itemsize == 4:
        src, out = a.view(np.uint32).reshape(-1), np.zeros(n * n, np.uint32)
        olib.ago_apply_symmetry(n, s, 0, ol.ptr(src), ol.ptr(out))
        return out.view(a.dtype)
    wide = np.ascontiguousarray(a.reshape(-1).astype(np.uint32))
    out = np.zeros(n * n, np.uint32)
    olib.ago_apply_symmetry(n, s, 0, ol.ptr(wide), ol.ptr(out))
    return out.astype(a.dtype)


def sample_stats(olib, game, index, n):
    """what the tests' non-vacuity conditions look at: proven wins / losses / draws among the entries, sum of visits, fillers"""
    visits, _, _, score, header = unpack(olib, game["samples"][index], n)
    pv = (score.astype(np.int32) >> 13) & 3
    proven = np.array([score_info(olib, x)[0] for x in score])
    entries = game["samples"][index][16:].reshape(-1, 6)
    return dict(wins=int((proven & (pv == 3)).sum()), losses=int((proven & (pv == 0)).sum()), draws=int((proven & (pv == 1)).sum()),
                draws_without_visits=int((proven & (pv == 1) & (visits == 0)).sum()), sum_visits=int(visits.sum()),
                filler=bool((entries[:, 0] == 255).any()) if entries.size else False, move_number=int(header[1]))


def reference_sample(olib, rules, n, game, index, augmentation, policy="torch_api"):
    """one sample -> dict(features u32[hw], policy f32[hw], value f32[3], moves_left f32[1], action_values f32[hw, 3])"""
    hw = n * n
    visits, _, value, score, header = unpack(olib, game["samples"][index], n)
    move_number = int(header[1])
    moves = game["moves"]
    board = np.zeros(hw, np.uint8)
    for i in range(move_number):   # Board::putMove
        m = int(moves[i])
        board[((m >> 2) & 127) * n + ((m >> 9) & 127)] = m & 3
    sign = int(moves[move_number]) & 3
    s = augmentation
    board = symmetric(olib, n, s, board)
    visits = symmetric(olib, n, s, visits)
    win = symmetric(olib, n, s, np.ascontiguousarray(value[:, 0]))
    draw = symmetric(olib, n, s, np.ascontiguousarray(value[:, 1]))
    score = symmetric(olib, n, s, score)
    features = np.zeros(hw, np.uint32)
    olib.ago_encode_features(rules, n, n, ol.ptr(np.ascontiguousarray(board)), sign, ol.ptr(features))

    policy_target, av = np.zeros(hw, np.float32), np.zeros((hw, 3), np.float32)
    policy_sum = F32(0.0)
    for i in range(hw):
        proven, pw, pd = score_info(olib, score[i])
        w, d = (pw, pd) if proven else (F32(win[i]), F32(draw[i]))
        av[i] = (w, d, F32(1.0) - (w + d))
        pv = (int(score[i]) >> 13) & 3
        if pv == 0:
            p = F32(1.0e-6)
        elif pv == 1:
            p = F32(int(visits[i])) if policy == "visits" else F32(max(1, int(visits[i])))
        elif pv == 3:
            p = F32(1.0e+6)
        else:
            p = F32(int(visits[i]))
        policy_target[i] = p
        policy_sum = F32(policy_sum + p)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = F32(1.0) / policy_sum
        policy_target = (policy_target * scale).astype(np.float32)
    outcome = game["outcome"]
    if outcome == 2:
        v = (1.0, 0.0) if sign == 1 else (0.0, 0.0)
    elif outcome == 3:
        v = (1.0, 0.0) if sign == 2 else (0.0, 0.0)
    else:
        v = (0.0, 1.0)
    value_target = np.array([v[0], v[1], F32(1.0) - (F32(v[0]) + F32(v[1]))], np.float32)
    return dict(features=features, policy=policy_target, value=value_target, moves_left=np.array([len(moves) - move_number], np.float32),
                action_values=av, sign=sign, board=board)


def input_planes(features, dtype=np.float32):
    """bit j of every feature word as 0 / 1: [..., 32]"""
    bits = (features[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.astype(dtype)


def reference_batch(olib, rules, n, fragments, samples, policy="torch_api", dtype=np.float32):
    """fragments: {index: [parsed games]}; samples: rows of (fragment, game, sample, augmentation)"""
    rows = [reference_sample(olib, rules, n, fragments[int(f)][int(g)], int(k), int(a), policy) for f, g, k, a in samples]
    feats = np.stack([r["features"] for r in rows])
    return dict(features=feats, input=input_planes(feats, dtype).reshape(len(rows), n, n, 32),
                policy_target=np.stack([r["policy"] for r in rows]).reshape(len(rows), n, n),
                value_target=np.stack([r["value"] for r in rows]), moves_left_target=np.stack([r["moves_left"] for r in rows]),
                action_values_target=np.stack([r["action_values"] for r in rows]).reshape(len(rows), n, n, 3))


def oracle_game(olib, rules, n, seed, sims=40, batch=4, max_steps=6000):
    """one self-play game of the oracle with its stand-in evaluator (ago_fake_eval), as GameDataStorage::serialize bytes"""
    cfg = ol.default_search_config(max_batch_size=batch, max_simulations=sims, table_entries=1 << 12)
    h = olib.ago_game_create(rules, n, n, ctypes.byref(cfg))
    op = np.zeros(64, np.uint16)
    k = olib.ago_prepare_opening(rules, n, n, seed, ol.ptr(op))
    olib.ago_game_begin(h, ol.ptr(op), k)
    feats = np.zeros((batch, n * n), np.uint32)
    for _ in range(max_steps):
        m = olib.ago_game_step_select(h, ol.ptr(feats), batch)
        pol, val = np.zeros((max(m, 1), n * n), np.float32), np.zeros((max(m, 1), 2), np.float32)
        olib.ago_fake_eval(m, n * n, ol.ptr(feats), ol.ptr(pol), ol.ptr(val))
        olib.ago_game_step_expand(h, ol.ptr(pol), ol.ptr(val))
        if olib.ago_game_outcome(h) != 0:
            break
    assert olib.ago_game_outcome(h) != 0, "the oracle game did not end"
    buf = np.zeros(1 << 20, np.uint8)
    size = olib.ago_game_storage_v201(h, ol.ptr(buf), buf.size)
    olib.ago_game_destroy(h)
    assert size > 0
    return buf[:size].copy()


def pack_sample(olib, n, stones, cells, visits, value, score, prior=None, root_score=UNKNOWN_SCORE, flags=0):
    """SearchDataStorage_v201::loadFrom + serialize (ago_sample_v201_pack) of hand-made root edges on `cells`"""
    cells = list(cells)
    moves = np.array([1 | ((c // n) << 2) | ((c % n) << 9) for c in cells], np.uint16)
    visits = np.ascontiguousarray(visits, dtype=np.int32)
    prior = np.ascontiguousarray(prior if prior is not None else np.full(len(cells), 1.0 / max(1, len(cells))), dtype=np.float32)
    value = np.ascontiguousarray(value, dtype=np.float32).reshape(len(cells), 2)
    score = np.ascontiguousarray(score, dtype=np.uint16)
    out = np.zeros(16 + 6 * n * n + 64, np.uint8)
    k = olib.ago_sample_v201_pack(n, n, stones, len(cells), ol.ptr(moves), ol.ptr(visits), ol.ptr(prior), ol.ptr(value), ol.ptr(score), root_score, flags,
                                  ol.ptr(out), out.size)
    assert k >= 16
    return out[:k].copy()


def move(sign, row, col):
    return sign | (row << 2) | (col << 9)


def crafted_game(olib, n, with_filler=False):
    """A hand-made game whose samples carry what self-play games may not supply: sample 0 (cross to move after 8 stones; cross holds two
    open twos that meet on (7, 7): a 3x3 fork, a foul under renju) with a proven win, a proven loss, a proven draw WITHOUT visits and an
    ordinary edge; sample 1 without any visits (proven edges only: storeTo takes the minimax value from the score); sample 2 with circle
    to move; with_filler (20x20): sample 3 whose only edge lies beyond cell 255, so that loadFrom inserts a filler entry."""
    moves = np.array([move(1, 7, 5), move(2, n - 1, 0), move(1, 7, 6), move(2, n - 1, 2), move(1, 5, 7), move(2, n - 1, 4), move(1, 6, 7), move(2, n - 1, 6),
                      move(1, 0, 0)], np.uint16)
    win_in, loss_in, draw_in, unknown = (lambda k: (3 << 13) | (4000 - k)), (lambda k: (0 << 13) | (4000 + k)), (lambda k: (1 << 13) | (4000 + k)), \
        (lambda e: (2 << 13) | (4000 + e))
    samples = [
        pack_sample(olib, n, 8, [20, 2 * n + 10, 2 * n + 11, 6 * n + 10], [0, 5, 0, 37], [[0.9, 0.05], [0.1, 0.2], [0.3, 0.6], [0.45, 0.25]],
                    [win_in(3), loss_in(2), draw_in(5), unknown(100)], root_score=win_in(4)),
        pack_sample(olib, n, 4, [30, 31], [0, 0], [[0.0, 0.0], [1.0, 0.0]], [loss_in(4), win_in(1)], root_score=win_in(2)),
        pack_sample(olib, n, 7, [3, n + 1, 4 * n + 4], [12, 3, 1], [[0.5, 0.1], [0.2, 0.7], [0.7, 0.6]], [unknown(0), unknown(-250), draw_in(9)]),
    ]
    if with_filler:
        samples.append(pack_sample(olib, n, 2, [300], [7], [[0.5, 0.1]], [unknown(0)]))
    return build_game(samples, moves, 2, n)
