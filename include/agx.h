/*
 * agx.h — C ABI of the MI355X-native self-play MCTS + policy/value evaluation engine.
 *
 * This is the drop-in boundary for the hot path of AlphaGomoku's src/search + src/selfplay +
 * src/networks. The reference has no FFI layer on this path (its boundary is a set of C++ classes over
 * the MinML C++ API), so the entry points below are what a cgo/ctypes/C++ facade for that path binds.
 * The only extern "C" surface in the reference is the dataset reader
 * include/alphagomoku/dataset/torch_api.h:13-43; its conventions are kept: plain structs, caller-owned
 * flat buffers, sizes queried first.  Unlike torch_api.h every call returns an int status (0 = ok) and
 * agx_last_error() returns the message — the C++ facade turns a non-zero status into the same
 * std::logic_error / std::runtime_error the reference throws (NNEvaluator.cpp:149,185-187).
 *
 * No torch types, no C++ types, no HIP types appear in the signatures.  Pointers named d_* are device
 * (HBM) addresses, h_* are host addresses, `stream` is a hipStream_t passed as void* (NULL = default).
 *
 * One handle per GPU, each driven by exactly one host thread (mirrors GeneratorThread,
 * src/selfplay/GeneratorManager.cpp:124-141).
 */
#ifndef AGX_H_
#define AGX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_OK 0
#define AGX_ERR_INVALID 1
#define AGX_ERR_HIP 2
#define AGX_ERR_UNSUPPORTED 3
#define AGX_ERR_STATE 4

/* Game rules, same numbering as ag::GameRules (include/alphagomoku/game/rules.hpp:18-25). */
enum AgxRules { AGX_FREESTYLE = 0, AGX_STANDARD = 1, AGX_RENJU = 2, AGX_CARO5 = 3, AGX_CARO6 = 4 };

/* Signs, same numbering as ag::Sign (include/alphagomoku/game/Move.hpp:17-23). */
enum AgxSign { AGX_NONE = 0, AGX_CROSS = 1, AGX_CIRCLE = 2, AGX_ILLEGAL = 3 };

const char* agx_last_error(void);
int agx_version(void);
/* sha256[:16] of the sources this library was compiled from (csrc + this header; alphagomoku_amd/build.py:source_hash) */
const char* agx_build_hash(void);
/* Selects the HIP device for the calling thread (one engine per GPU). */
int agx_set_device(int device);
int agx_device_count(int* count);
int agx_device_cu_count(int* count); /* compute units of the current device */

/* ------------------------------------------------------------------------------------------------
 * Policy/value network (replaces AGNetwork::forward / asyncForwardLaunch+Join over ml::Graph,
 * src/networks/AGNetwork.cpp:61-88, for the ResnetPV architecture of src/networks/networks.cpp:71-93
 * built from src/networks/blocks.cpp:32-38,45-55,99-118 after optimize(2) has folded the BNs).
 * ---------------------------------------------------------------------------------------------- */
typedef struct AgxNetDesc
{
	int rows;           /* board rows, 5 .. 20 */
	int cols;           /* board cols, 5 .. 20, independent of rows (15x15 and 20x20 run kernels of their own, every other shape the
	                       run-time-shaped one, csrc/nn_any_board.hip; AGX_NN_ANY_BOARD=1 in the environment sends those two there as well) */
	int blocks;         /* residual blocks */
	int filters;        /* conv filters F: 64 or 128 for every architecture (one LDS-resident plane per board); the residual networks
	                       (AGX_ARCH_RESNET) also take 192, 256, ... 512 (multiples of 64), which run a launch per layer with the activations
	                       in a global scratch (csrc/nn_layered.hip; AGX_NN_LAYERED=1 in the environment sends 64 and 128 there as well) */
	int in_channels;    /* 32 (bit-packed features, NNInputFeatures.cpp:59-113) or 8 (ResnetPVraw, networks.cpp:107-129: ml::unpackInput
	                       expands the 8 low bits of the feature word, AGNetwork.cpp:249-258; without the action-values head) */
	int value_hidden;   /* D = min(256, 2F) (blocks.cpp:113) */
	int action_values;  /* 0: ResnetPV (outputs "pv", networks.cpp:71-93); 1: ResnetPVQ (:143-168) with the action-values head 'q' */
} AgxNetDesc;

typedef struct AgxNet AgxNet; /* opaque */

/* Number of fp32 values in the canonical (BN-folded) weight blob — one layout for every filter count F, 64 to 512 —, in this order:
 *   conv_in  W[5][5][Cin][F]  b[F]
 *   blocks x { W1[3][3][F][F] b1[F]  W2[3][3][F][F] b2[F] }
 *   policy   Wp1[3][3][F][F] bp1[F]  Wp2[F] bp2[1]
 *   value    Wv1[F][4] bv1[4]  Wv2[rows*cols*4][D] bv2[D]  Wv3[D][3] bv3[3]
 *   action values (only with desc.action_values; createActionValuesHead, blocks.cpp:119-127):
 *            Wq1[3][3][F][F] bq1[F] (tanh)  Wq2[F][3] bq2[3] (softmax over the 3 outputs of every cell)
 * Conv weights are [kh][kw][cin][cout] (cross-correlation, "same" zero padding); the value-head flatten
 * order is NHWC row-major: index = (row*cols + col)*4 + c.  */
size_t agx_net_blob_floats(const AgxNetDesc* desc);
int agx_net_create(const AgxNetDesc* desc, AgxNet** out);
/* Packs and uploads the blob; may be called again on a network in use (it waits for the device before the old weights go).  A blob of the
 * wrong length is AGX_ERR_INVALID before anything is touched.  A reload that fails later (an allocation, a copy) leaves the weights loaded
 * before it in place, for every architecture: the new ones are complete on the device before the old ones are let go. */
int agx_net_load_weights(AgxNet* net, const float* h_blob, size_t n_floats);
/* d_features: uint32[batch][rows*cols] (one bit-packed word per cell);
 * d_policy: float[batch][rows*cols] (softmax over the board); d_value: float[batch][3] = (win, draw, loss). */
int agx_nn_forward(AgxNet* net, const uint32_t* d_features, int batch, float* d_policy, float* d_value, void* stream);
/* ResnetPVQ: additionally d_action_values float[batch][rows*cols][2] = (win, draw) of the per-cell softmax-3 'q' output, the part
 * NetworkDataPack::unpackActionValues keeps (NetworkDataPack.cpp:214-224).  Passing NULL skips the head. */
int agx_nn_forward_pvq(AgxNet* net, const uint32_t* d_features, int batch, float* d_policy, float* d_value, float* d_action_values, void* stream);
int agx_net_description(const AgxNet* net, AgxNetDesc* out);
/* Caps the persistent grid of the tower kernel at `workgroups` CUs (0 = all of them).  A tower workgroup fills its CU (LDS, registers), so
 * a narrowed launch leaves whole CUs to kernels running at the same time on other streams: the other slices of a pool stepped as
 * pipelined groups (agx_engine_*_group).  The layered towers (filters above 128) cap every layer's grid at the workgroups that fill that
 * many CUs. */
int agx_net_set_launch_width(AgxNet* net, int workgroups);
int agx_net_destroy(AgxNet* net);

/* Same network, but the batch is a device-side list: position i is slot d_slot_list[i] of the slot-indexed buffers
 * (features uint32[slots][cells], policy float[slots][cells], value float[slots][3]); the batch size is read from
 * *d_count on the device, so no host synchronisation is needed between the search kernels and the network
 * (replaces NNEvaluator::pack_to_network / asyncEvaluateGraphLaunch, src/search/monte_carlo/NNEvaluator.cpp:182-262). */
int agx_nn_forward_indirect(AgxNet* net, const uint32_t* d_features, const int* d_slot_list, const int* d_count, int max_batch,
		float* d_policy, float* d_value, void* stream);
int agx_nn_forward_indirect_pvq(AgxNet* net, const uint32_t* d_features, const int* d_slot_list, const int* d_count, int max_batch,
		float* d_policy, float* d_value, float* d_action_values, void* stream);

/* ConvNeXt networks: ConvNextPVQraw (networks.cpp:1078-1140) and ConvNextPVQMraw (:1142-1219, with the moves-left output 'm').  AgxNetDesc
 * keeps its seven ints; the architecture and the moves-left head are named next to it.  For AGX_ARCH_CONVNEXT the description must have
 * in_channels 8 (the 8 low bits of the feature word), action_values 1, value_hidden 256 and filters 64 or 128, on boards 5..20 x 5..20.
 * The network after the batch norms are folded (F = filters, HW = rows * cols):
 *   conv_in  5x5, 8 -> F, + b, relu
 *   blocks x y = depthwise 7x7 (x) + bd ; y = relu(W1 . y + b1) ; x = W2 . y + b2 + x (no activation) ;
 *            x = x * sigmoid(Ws2 . relu(Ws1 . mean_hw(x) + bs1) + bs2) per channel
 *   policy   relu(Wp1 . x + bp1) ; Wp2 . + bp2 (F -> 1) ; softmax over the board
 *   value    relu(Wv1 . x + bv1) ; mean_hw ; relu(Wv2 . + bv2) (F -> 256) ; Wv3 . + bv3 (256 -> 3) ; softmax
 *   q        relu(Wq1 . x + bq1) ; Wq2 . + bq2 (F -> 3) ; softmax per cell
 *   m        relu(Wm1 . x + bm1) (F -> 32) ; mean_hw ; relu(Wm2 . + bm2) (32 -> 128) ; Wm3 . + bm3 (128 -> HW) ; softmax
 * The canonical fp32 blob holds, in this order:
 *   conv_in  W[5][5][8][F] b[F]
 *   blocks x { Wd[7][7][F] bd[F]  W1[F][F] b1[F]  W2[F][F] b2[F]  Ws1[F][F] bs1[F]  Ws2[F][F] bs2[F] }
 *   policy   Wp1[F][F] bp1[F]  Wp2[F] bp2[1]
 *   value    Wv1[F][F] bv1[F]  Wv2[F][256] bv2[256]  Wv3[256][3] bv3[3]
 *   q        Wq1[F][F] bq1[F]  Wq2[F][3] bq2[3]
 *   m (only with moves_left)  Wm1[F][32] bm1[32]  Wm2[32][128] bm2[128]  Wm3[128][HW] bm3[HW]
 * 1x1 convolutions and dense layers are [in][out]; the depthwise convolution is a cross-correlation with "same" zero padding.
 *
 * Bottleneck networks: BottleneckPV, BottleneckPVraw and BottleneckPVQ (networks.cpp:170-361; blocks of createBottleneckBlock_v3,
 * blocks.cpp:84-97).  For AGX_ARCH_BOTTLENECK the description is the residual networks': rows and cols 5..20, filters F 64 or 128 (the inner
 * width is F/2), blocks >= 0, value_hidden min(256, 2F), in_channels 32, or 8 without the action-values head; moves_left 0.  Input block and
 * heads are the residual networks'.  The canonical fp32 blob after the batch-norm fold:
 *   conv_in  W[5][5][Cin][F] b[F]
 *   blocks x { W1[F][F/2] b1[F/2]   W2[3][3][F/2][F/2] b2[F/2]   W3[3][3][F/2][F] b3[F] }
 *            y = relu(W1.x + b1) ; y = relu(W2*y + b2) ; x = relu(x + W3*y + b3)
 *   policy / value / action values: exactly the residual networks' parts (above), in their order */
enum AgxNetArchitecture { AGX_ARCH_RESNET = 0, AGX_ARCH_CONVNEXT = 1, AGX_ARCH_BOTTLENECK = 2 };
size_t agx_net_blob_floats_ex(const AgxNetDesc* desc, int architecture, int moves_left); /* 0 for a combination that does not exist */
/* architecture AGX_ARCH_RESNET with moves_left 0 is agx_net_create.  What the kernels do not cover is AGX_ERR_UNSUPPORTED with a message.
 * Every entry point that takes an AgxNet takes the result: agx_net_load_weights (the blob above), agx_nn_forward[_indirect][_pvq],
 * agx_net_set_launch_width, agx_net_description, agx_net_destroy, and with them the pool, the position evaluators and searchers and
 * agx_net_score_dataset*. */
int agx_net_create_ex(const AgxNetDesc* desc, int architecture, int moves_left, AgxNet** out);
int agx_net_architecture(const AgxNet* net, int* architecture, int* moves_left);
/* agx_nn_forward[_indirect]_pvq with the moves-left output: d_moves_left float[batch or slots][rows*cols], the softmax of the 'm' head (index i
 * = i moves left, NetworkDataPack.cpp:224-235).  d_action_values and d_moves_left may each be NULL (head skipped); a d_moves_left on a
 * network without the head is AGX_ERR_INVALID. */
int agx_nn_forward_pvqm(AgxNet* net, const uint32_t* d_features, int batch, float* d_policy, float* d_value, float* d_action_values,
		float* d_moves_left, void* stream);
int agx_nn_forward_indirect_pvqm(AgxNet* net, const uint32_t* d_features, const int* d_slot_list, const int* d_count, int max_batch,
		float* d_policy, float* d_value, float* d_action_values, float* d_moves_left, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Device-resident self-play engine: a pool of independent games, each with its own search tree, solver transposition
 * table and task buffer in HBM.  Replaces, for one GeneratorThread (src/selfplay/GeneratorManager.cpp:124-141), the
 * per-game objects GameGenerator{Game, Tree, Search{AlphaBetaSearch}} and their calls
 *   Search::select / solve / scheduleToNN / generateEdges / expand / backup / cleanup   (Search.hpp:78-90)
 *   Tree::setBoard / select / expand / backup / getInfo                                   (Tree.hpp:68-104)
 *   GameGenerator::generate / make_move / prepare_search                                  (GameGenerator.cpp:46-185)
 * Configuration fields carry the reference's names (utils/configs.hpp: GameConfig, TreeConfig, EdgeSelectorConfig,
 * MCTSConfig, TSSConfig, SearchConfig, SelfplayConfig::constraints.max_simulations).
 * ---------------------------------------------------------------------------------------------- */
typedef struct AgxEngineConfig
{
	int rules;                        /* AgxRules (all five rule sets run on the device) */
	int board_size;                   /* square boards, <= 20 */
	int draw_after;                   /* GameConfig::draw_after, <= 0 means rows*cols */
	int n_games;                      /* games resident on this GPU (SelfplayConfig::games_per_thread) */
	int max_batch_size;               /* SearchConfig::max_batch_size: simulations selected per game per step */
	int max_simulations;              /* SelfplayConfig::constraints.max_simulations (playouts per move).  Keep it >= 50: with a drawish root the
	                                     move rule asks for max - clamp((draw - 0.75) / 0.25) * (max - 50) visits (utils/misc.cpp:171-179), which
	                                     EXCEEDS max below 50 while select stops at max — such a game never moves, here as in the reference. */
	float exploration_constant;       /* EdgeSelectorConfig */
	float exploration_scaling;
	int init_to;                      /* 0 "q_head", 1 "parent", 2 "draw", 3 "loss" */
	float information_leak_threshold; /* TreeConfig */
	float policy_expansion_threshold; /* MCTSConfig */
	int tss_max_positions;            /* TSSConfig::max_positions, <= 1000 (the search depth is capped at 100 plies either way) */
	uint64_t tss_table_entries;       /* AlphaBetaSearch's SharedHashTable size per game (reference: 4 Mi) */
	uint64_t zobrist_seed;            /* seed of the solver / node-cache Zobrist keys (the reference draws them from a time-seeded RNG) */
	int node_capacity;                /* per game, per arena, size class 0 (TreeConfig::node_bucket_size analogue; see arena_reserve) */
	int edge_capacity;                /* per game, per arena, size class 0 (TreeConfig::edge_bucket_size analogue).  The arenas grow on demand
	                                     like the reference's pools (arena_reserve below) */
	int record_capacity;              /* move records kept on the device, 0 = n_games * cells */
	int record_edge_capacity;         /* root-edge snapshots kept on the device, 0 = 64 per record */
	float solver_yield_fraction;      /* 0 = off.  A pool step lasts as long as its slowest game's solver batch; with f in (0,1] a game
	                                     whose batch is only partly solved when a fraction f of the launch's games are done sits out the
	                                     rest of this step (network / expand) and resumes in the next one.  Per-game results are
	                                     unchanged (every game executes the same sequence of operations), only the pacing differs. */
	int final_selector;               /* GameGenerator::make_move's EdgeSelector (SelfplayConfig::final_selector.policy): 0 "best",
	                                     1 "max_visit", 2 "min_visit", 3 "max_value", 4 "max_policy", 5 "lcb" with exploration_constant
	                                     (EdgeSelector.cpp:446-536) */
	int use_symmetries;               /* NNEvaluator::useSymmetries (NNEvaluator.cpp:134-141,244-286): every position handed to the network
	                                     is augmented by one of the 8 board symmetries and the policy is mapped back.  The reference draws
	                                     randInt(8) from a time-seeded generator; here the k-th position of game `serial` uses
	                                     splitmix64(symmetry_seed ^ serial << 32 ^ k) >> 61, so runs are reproducible. */
	uint64_t symmetry_seed;
	int max_children;                 /* MCTSConfig::max_children: non-root nodes keep at most this many edges (the best by proven score, then
	                                     prior) and of those only the ones with prior >= policy_expansion_threshold * (their prior sum)
	                                     (prune_weak_moves, EdgeGenerator.cpp:49-86).  0 = unlimited, the reference default. */
	int noise_type;                   /* EdgeSelectorConfig::noise_type at the root: 0 "none", 1 "custom", 2 "dirichlet" (alpha 0.05), 3 "gumbel"
	                                     (create*Noise, utils/random.cpp:89-124; mixed into the priors as EdgeSelector.cpp:602-623 does).
	                                     Drawn once per move by the first select that sees an expanded root, like the selector that
	                                     prepare_search creates per move.  Stream: counter-based hash of (noise_seed, game serial, move
	                                     number) — the reference uses a time-seeded mt19937; log / exp are fixed double-precision series
	                                     (csrc/root_noise.hpp), so runs are reproducible and identical on host and device. */
	float noise_weight;
	uint64_t noise_seed;
	int action_values;                /* 1: the network is a 'pvq' network (AGNetwork::getOutputConfig): agx_engine_evaluate runs its
	                                     action-values head and new edges start from those values (initialize_edges, EdgeGenerator.cpp:
	                                     119-124) — what the default init_to = "q_head" selector reads.  0: 'pv' network, edges start
	                                     at (0, 0) exactly as the reference's zero-filled 'q' tensor gives (NetworkDataPack.cpp:122-126). */
	int match_mode;                   /* 1: evaluation matches (evaluation/EvaluationGame.cpp, evaluation/Player.cpp).  n_games must be even:
	                                     tree g < n_games/2 belongs to the first player of match g, tree g + n_games/2 to the second player;
	                                     both see one game and a tree searches only on its own player's turns (Player::setBoard jumps two
	                                     plies; trees persist across games, the solver table is cleared per game; the root is pruned like
	                                     any other node, UnifiedGenerator's forceExpandRoot = false).  Every opening is played twice with
	                                     the colours swapped.  Drive it with agx_engine_step_match(e, first_net, second_net, s), or with two
	                                     groups on ONE stream: agx_engine_step_group(e, first_net, 0, 2, s); ..._group(e, second_net, 1, 2, s). */
	float policy_temperature;         /* MCTSConfig::policy_temperature (initialize_edges, EdgeGenerator.cpp:88-127): 1 = priors are the policy
	                                     (reference default); 0 = prior 1 for the cells that hold the policy maximum, 0 elsewhere; otherwise
	                                     policy^(1/T), evaluated as exp(log(p)/T) with the fixed double-precision series of csrc/root_noise.hpp
	                                     (the reference calls std::pow), so device and oracle agree bit for bit. */
	float arena_reserve;              /* the tree arenas are regions of pool-wide heaps sized n_games x (class-0 bundle) x (1 + arena_reserve).
	                                     node_capacity / edge_capacity are the CLASS-0 sizes every game starts with; a game whose batch would
	                                     not fit moves into a bundle of twice the size from the reserve (NodeCache::resize x2, NodeCache.cpp:
	                                     320-355; ObjectPool growth, utils/ObjectPool.hpp:74-289) — it sits out one expand stage, its results do
	                                     not change — and hands it back when its game is over.  Only with the reserve exhausted (or beyond 32 x
	                                     the class-0 size) does an overflowing tree stop its game (agx_engine_stats.first_error).  < 0 = default 1.0 */
	int search_threads;               /* > 1: tournament search (player/SearchThread.cpp:121-180): the pool is ONE game tree searched by
	                                     `search_threads` SearchThreads, each with its own Search — own task buffer of max_batch_size leaves, own
	                                     threat solver and table — and n_games must equal search_threads (record 0 owns the tree, the others are the
	                                     threads).  Per step the threads take the tree in thread order for select (virtual loss makes them spread),
	                                     solve their batches in parallel (one wave each), share one network launch, then take the tree in order
	                                     again for expand + backup: the lock-step interleaving of SearchThread::serial_run.  0 / 1 = self-play pool. */
	int record_format;                /* what k_advance keeps of every played move's root (SearchDataPack, dataset/data_packs.cpp:24-43):
	                                     bit 0 (value 1, the default): the root edges as 24-byte AgxEdgeView snapshots;
	                                     bit 1 (value 2): the sample quantised on the device to dataset format 201
	                                     (SearchDataStorage_v201::loadFrom + serialize, dataset/SearchDataStorage.cpp:326-374,410-419:
	                                     16-byte header + 6 bytes per visited / proven cell) — a quarter of the bytes to keep and copy;
	                                     3 = both.  Finished games are always reported (AgxGameEnd). */
	int record_sample_capacity;       /* bytes of the format-201 sample pool, 0 = room for an entry on every cell of every record (capped at 2 GiB) */
	int game_end_capacity;            /* finished-game records kept on the device, 0 = max(2 * n_games, record_capacity / 16) */
	int speculative_solver;           /* 1: agx_engine_select_solve* runs select + threat solver as ONE persistent launch (k_search_spec) in which the
	                                     leaves of a game's batch are solved in PARALLEL, each wave against the game's transposition table as it was
	                                     before the batch (every touched bucket copied into a per-task overlay), and committed in batch order; a task
	                                     that saw a bucket an earlier task of the batch changed is solved again serially — results are bit-identical
	                                     to the serial order of Search::solve (Search.cpp:159-183), the solver runs with 3-4 waves per SIMD instead of
	                                     one wave per game.  0 (default): one wave per game, tasks in order.  Tournament-search pools (search_threads > 1)
	                                     take the speculative launch too; ignored for solver budgets above 250 positions (the overlay
	                                     holds 256 buckets) and batches above 16. */
	int speculative_waves;            /* waves of that launch over the whole pool, 0 = as many as stay resident: 16 per compute unit of the device on 15x15
	                                     boards, 10 on 20x20 (agx_engine_speculative_waves reports the number in use) */
	int force_expand_root;            /* UnifiedGenerator's forceExpandRoot (EdgeGenerator.cpp:283-285): 1 (default, self-play: GameGenerator.cpp:183-184)
	                                     never prunes the root's edges; 0 prunes the root like any node (evaluation Player, Player.cpp:109; match_mode
	                                     engines always do) */
	int search_buffers;               /* 2: the double-buffered tournament search of SearchThread::asynchronous_run (player/SearchThread.cpp:148-180,
	                                     Search::useBuffer / switchBuffer, Search.cpp:243-252): every search thread has TWO task buffers, one solver
	                                     and table; n_games must equal 2 x max(search_threads, 1) and record b * threads + t is buffer b of thread t.
	                                     The pool is stepped buffer by buffer as group b of 2 (agx_engine_expand_backup_group, then
	                                     agx_engine_select_solve_group, then the network on that group): the leaves of buffer b stay in the network
	                                     — virtual losses applied — while buffer 1 - b is expanded, backed up, selected and solved, which is the
	                                     overlap of tower and tree work inside ONE game that the reference gets from asyncEvaluateGraphLaunch / Join.
	                                     When the move rule fires after a buffer's backup, the other buffer's leaves are dropped and their virtual
	                                     losses taken back (Search::cleanup).  Also valid with search_threads 0 / 1 (one thread, two buffers — the
	                                     reference's "1 thread per GPU" setting).  0 / 1 (default): one buffer. */
} AgxEngineConfig;

typedef struct AgxEngine AgxEngine; /* opaque */

typedef struct AgxEngineBuffers
{
	uint32_t* d_nn_features; /* [slots][cells] */
	float* d_nn_policy;      /* [slots][cells] */
	float* d_nn_value;       /* [slots][3] */
	float* d_nn_action_values; /* [slots][cells][2] = (win, draw) per cell; read only when AgxEngineConfig.action_values is set */
	int* d_nn_list;          /* slots scheduled for evaluation by the last agx_engine_select_solve */
	int* d_nn_count;         /* number of entries of d_nn_list */
	int slots;
	int cells;
} AgxEngineBuffers;

typedef struct AgxEngineStats
{ /* SearchStats counters (Search.hpp:33-54) summed over the pool + pool-level counters */
	unsigned long long evaluated_nodes;       /* nb_node_count: simulations backed up */
	unsigned long long network_evaluations;   /* nb_network_evaluations */
	unsigned long long information_leaks;     /* nb_information_leaks */
	unsigned long long proven_edge_visits;    /* nb_proven_states */
	unsigned long long wasted_expansions;     /* nb_wasted_expansions */
	unsigned long long duplicate_selections;  /* nb_duplicate_nodes */
	unsigned long long solver_nodes;          /* positions visited by the alpha-beta solver */
	unsigned long long select_levels;         /* tree levels descended by select (incl. dropped leak descents) */
	unsigned long long select_edge_reads;     /* edges scanned by PUCT argmax */
	unsigned long long moves_played;
	unsigned long long peak_nodes;            /* largest per-game node / edge arena use seen */
	unsigned long long peak_edges;
	int games_finished;
	int openings_taken;
	int active_games;
	int records_used;
	int record_edges_used;
	int first_error;                          /* 0 = none; EngineError of the first game that stopped */
	int arena_grows;                          /* bundles handed out by the arena heap to games that outgrew theirs */
	int arena_releases;                       /* grown bundles handed back by finished games */
	int arena_failures;                       /* growth requests the heap could not serve (reserve exhausted) */
	int arena_max_class;                      /* largest size class in use: capacities = class-0 capacities << class */
	float arena_heap_used;                    /* high-water mark of the edge heap, fraction of its size */
	int speculative_parks;                    /* speculative solves set aside at the end of a launch and taken up again by the next one (engine: "Parking") */
	unsigned long long speculative_solves;    /* speculative_solver: leaves solved against the pre-batch table ... */
	unsigned long long speculative_reruns;    /* ... and how many of them had to be solved again serially (conflict or full overlay) */
	unsigned long long speculative_deferrals; /* batches whose commit was put off to the next launch (solver_yield_fraction) */
} AgxEngineStats;

typedef struct AgxEdgeView
{ /* ag::Edge (Edge.hpp:23-32) */
	float prior, win, draw;
	int32_t visits;
	uint16_t move;   /* Move::toShort: sign | row << 2 | col << 9 */
	uint16_t score;  /* Score raw bits */
	uint16_t flag_and_virtual_loss;
	uint16_t reserved;
} AgxEdgeView;

typedef struct AgxGameInfo
{
	int active, sign_to_move, n_moves, outcome, error, opening_id, games_done, n_nodes, n_edges;
	int root_visits;
	float root_win, root_draw;
	int root_score;
	int root_edges;
	int grow_pending; /* non-zero: the game's last batch waits for its expansion in larger arenas (one step later than a lock-step pool) */
	int arena_class;  /* its tree arenas hold class-0 capacity << arena_class records */
	float root_moves_left; /* Tree::getMovesLeft (Tree.cpp:173-176, :350): the root's running mean of the moves-left estimates backed up through it */
	int max_depth;         /* Tree::getMaximumDepth (Tree.cpp:188-191): longest select path that reached a leaf since the last setBoard */
} AgxGameInfo;

typedef struct AgxMoveRecord
{ /* one self-play sample: SearchDataPack(const Node&, board) (dataset/data_packs.cpp:24-43) */
	int game_serial, move_number;
	uint16_t move, root_score;
	int root_visits;
	float root_win, root_draw;
	int n_edges, edge_offset;
	int root_flags; /* SearchDataPack::flags: bit 0 root statically solved, 1 recursively solved, 2 must defend (data_packs.cpp:40-42) */
	int game_slot;      /* the pool slot (tree) that produced the sample */
	int game_index;     /* games that slot had finished before this one: (game_slot, game_index) identifies a game; game_serial is the
	                       opening id, which the two colour-swapped games of a match share */
	int sample_offset;  /* record_format bit 1: the format-201 bytes of this sample inside the sample pool (-1 = not recorded) */
	int sample_bytes;
	int outcome;        /* GameOutcome after this move (0 unknown / 1 draw / 2 cross win / 3 circle win): non-zero on a game's last move */
} AgxMoveRecord;

typedef struct AgxGameEnd
{ /* one finished game: what GameGenerator::generate passes on when Game::isOver (GameGenerator.cpp:104-114) */
	int game_serial, game_slot, game_index;
	int outcome;         /* GameOutcome (game/rules.hpp:29-35) */
	int n_moves;         /* Game::getMoves(): opening stones included */
	uint16_t moves[400]; /* Move::toShort */
} AgxGameEnd;

typedef struct AgxSavedGame
{ /* one game in flight, as GameGenerator::save keeps it (selfplay/GameGenerator.cpp:122-130: Game::serialize + the samples so far — the samples
     stay with the AgxGameBuffer, see agx_game_buffer_take_pending): search trees are not checkpointed */
	int game_slot, game_index;   /* the pool slot and the number of games it had finished (the key of the game's pending samples) */
	int opening_id, sign_to_move, nn_queued, n_moves;
	uint16_t moves[400];         /* Move::toShort, opening stones included */
} AgxSavedGame;

typedef struct AgxRecordCounts
{
	int records, edges, sample_bytes, game_ends;
} AgxRecordCounts;

#define AGX_OPENING_CAP 32 /* uint16 per opening: [0] = number of stones, [1..] = Move::toShort */

/* Host-only: one synthetic random opening with the distribution of the reference's prepareOpening (utils/misc.cpp:142-170);
 * h_opening receives AGX_OPENING_CAP words ([0] = stones, then Move::toShort, cross first). */
int agx_make_opening(int rules, int board_size, uint32_t seed, uint16_t* h_opening);
/* Host-only: getOutcome (src/game/rules.cpp:110-133) after the stone `sign` was put on (row, col) of h_board (board_size^2
 * bytes, 0 empty / 1 cross / 2 circle, the stone already on it): 0 unknown, 1 draw, 2 cross win, 3 circle win.  Under renju a
 * foul of cross (isForbidden, rules.cpp:134-173) is a circle win.  draw_after <= 0 means "full board".  The same test runs on
 * the device after every played move; this entry point is what openings and host-side callers use. */
int agx_get_outcome(int rules, int board_size, const uint8_t* h_board, int sign, int row, int col, int draw_after, int* outcome);

int agx_engine_default_config(AgxEngineConfig* cfg);
int agx_engine_create(const AgxEngineConfig* cfg, AgxEngine** out);
int agx_engine_destroy(AgxEngine* engine);
/* OpeningGenerator::generate (selfplay/OpeningGenerator.cpp:21-78) for `count` openings, batched on the device: candidates from
 * agx_make_opening(seed, seed + 1, ...) that the threat solver cannot prove within 1000 nodes are evaluated by `net` and accepted
 * when |expectation - 0.5| < 0.1 + 0.01 * trials.  h_openings receives count x AGX_OPENING_CAP words (the layout agx_engine_begin
 * takes); h_stats (optional, 4 ints): candidates drawn, proven by the solver, rejected as unbalanced, network evaluations.
 * Borrows the pool's task slots: only valid before agx_engine_begin. */
int agx_engine_generate_openings(AgxEngine* engine, AgxNet* net, int count, uint32_t seed, uint16_t* h_openings, int* h_stats);
/* Starts every game of the pool from h_openings[n_openings][AGX_OPENING_CAP]; finished games take the next unused opening. */
int agx_engine_begin(AgxEngine* engine, const uint16_t* h_openings, int n_openings, void* stream);
/* One pool step = select_solve -> evaluate -> expand_backup.  The three stages are exposed separately so that a caller
 * (or a test) can run any evaluator over AgxEngineBuffers between them. */
int agx_engine_select_solve(AgxEngine* engine, void* stream);
int agx_engine_evaluate(AgxEngine* engine, AgxNet* net, void* stream);
int agx_engine_expand_backup(AgxEngine* engine, void* stream);
int agx_engine_step(AgxEngine* engine, AgxNet* net, void* stream);
/* The same stages restricted to group `group` of `n_groups` equal slices of the pool.  Games are independent, so slices can be
 * driven from different streams and drift apart: while one slice waits for its slowest solver wave, the others use the CUs
 * (at most 16 groups).  Results per game do not depend on the grouping.  A network may be shared by the slices: the single-plane
 * kernels keep their scratch per stream. */
int agx_engine_select_solve_group(AgxEngine* engine, int group, int n_groups, void* stream);
/* the two halves of select_solve separately: Search::select, then Search::solve + scheduleToNN (Search.hpp:78-82) */
int agx_engine_select_group(AgxEngine* engine, int group, int n_groups, void* stream);
int agx_engine_solve_group(AgxEngine* engine, int group, int n_groups, void* stream);
int agx_engine_evaluate_group(AgxEngine* engine, AgxNet* net, int group, int n_groups, void* stream);
int agx_engine_expand_backup_group(AgxEngine* engine, int group, int n_groups, void* stream);
/* the two halves of expand_backup separately: Search::generateEdges + expand + backup (Search.hpp:84-86), then GameGenerator::make_move +
 * prepare_search for the games whose search is complete and the next openings for the games that ended (GameGenerator.cpp:97-118,145-185) */
int agx_engine_expand_group(AgxEngine* engine, int group, int n_groups, void* stream);
int agx_engine_advance_group(AgxEngine* engine, int group, int n_groups, void* stream);
int agx_engine_step_group(AgxEngine* engine, AgxNet* net, int group, int n_groups, void* stream);
int agx_stream_create(void** out_stream);
/* A stream whose kernels run only on the compute units set in the mask (bit i = compute unit i).  A pool stepped as N slices
 * (agx_engine_*_group) on N such streams with disjoint masks — 4 x 64 CUs on MI355X — runs its slices out of phase, each on its own part
 * of the chip: the power-limited network launches never cover the whole chip at once and hold a higher clock, and no slice waits for
 * another's stragglers (+10 % simulations/s).  Narrow the network's persistent grid to the slice's CU count
 * (agx_net_set_launch_width).  Do not destroy such a stream while the process lives (hipStreamDestroy of a CU-masked stream hangs on
 * ROCm 7.2): agx_stream_destroy leaves them to process exit. */
int agx_stream_create_with_cu_mask(void** out_stream, const uint32_t* cu_mask, int n_words);
/* the same, for callers that need several streams on one mask (the slices of a pool sharing the search partition of the chip): streams are
 * cached by (device, mask, instance); instance 0 is what agx_stream_create_with_cu_mask returns */
int agx_stream_create_with_cu_mask_instance(void** out_stream, const uint32_t* cu_mask, int n_words, int instance);
/* events order launches across streams on the device (hipStreamWaitEvent): record on one stream, make another wait for it */
int agx_event_create(void** out_event);
/* host pacing: a launch loop that runs ahead of the device without bound ends up spinning on a full launch queue (a whole CPU per rank).  Record a
 * BLOCKING event behind every step and wait for the one N steps back: the host thread sleeps, the device stays N steps fed
 * (measured: 1.98 -> 0.12 CPUs per rank, simulations/s +1 %; agx.hpp: HostPacer).  agx_event_synchronize SLEEPS: it polls the event between
 * 100 us naps (hipEventSynchronize spins in user space on ROCm 7.2 even for a hipEventBlockingSync event). */
int agx_event_create_blocking(void** out_event);
int agx_event_synchronize(void* event);
int agx_event_record(void* event, void* stream);
int agx_stream_wait_event(void* stream, void* event);
int agx_event_destroy(void* event);
/* streams agx_stream_create_with_cu_mask has created in this process: they are cached by (device, mask) and handed out again, never destroyed */
int agx_stream_masked_count(void);
int agx_stream_destroy(void* stream);
int agx_stream_synchronize(void* stream);
/* One game driven from OUTSIDE, the way evaluation/Player.cpp:100-129 drives a Tree / Search pair: agx_engine_set_board is
 * Search::cleanup + Tree::setBoard(board, signToMove) + Search::setBoard (Tree.cpp:128-151: the cached states still reachable from the new
 * position are kept, the root is the cached node of the position if there is one; the solver table ages by a generation); the caller then
 * steps select_solve / evaluate / expand (agx_engine_expand_group: no move is played by the engine) until ITS stopping rule says so, reads the
 * root (agx_engine_game_info) and decides the move.  h_board: one byte per cell, 0 empty / 1 cross / 2 circle.  This is
 * Tree::setBoard(board, sign, forceRemoveRootNode = false); agx_engine_set_board_ex takes the flag.  agx_engine_set_max_simulations: the
 * budget Search::select(tree, maxSimulations) takes per call. */
int agx_engine_set_board(AgxEngine* engine, int game, const uint8_t* h_board, int sign_to_move, void* stream);
/* Tree::setBoard(board, sign, forceRemoveRootNode) (Tree.cpp:145-147): with force_remove_root != 0 the cached node of the new position itself
 * is dropped while the tree is rebased (its former children stay cached), so the root is absent and the next select stage hands the position
 * to the network afresh — what the analysis engine does on every new position (player/SearchEngine.cpp:97-104).  force_remove_root = 0 is
 * agx_engine_set_board. */
int agx_engine_set_board_ex(AgxEngine* engine, int game, const uint8_t* h_board, int sign_to_move, int force_remove_root, void* stream);
int agx_engine_set_max_simulations(AgxEngine* engine, int max_simulations);
/* Search::setBatchSize (search/monte_carlo/Search.cpp:252-255; SearchThread.cpp:125-126 grows it with sqrt(simulations)): the number of leaves the
 * select stage takes per game from the next launch on, 1 .. max_batch_size (the capacity the engine was created with) */
int agx_engine_set_batch_size(AgxEngine* engine, int batch_size);
/* Search::cleanup (search/monte_carlo/Search.cpp:233-242): the leaves that were selected but not expanded — in every task buffer, of every
 * tree of the engine — are dropped and their virtual losses taken back (Tree::cancelVirtualLoss, Tree.cpp:377-384).  agx_engine_set_board does
 * this for its game by itself; a caller that stops a double-buffered search (SearchThread.cpp:108-109) calls it before reading the tree. */
int agx_engine_cancel_pending(AgxEngine* engine, void* stream);
/* Tree::getSimulationCount / isRootProven / getNodeCount (Tree.hpp:86-92) as a search loop reads them between two steps (the stop condition of
 * player/SearchThread.cpp:181-199): out4 = { root visits, root proven (0 / 1), nodes in the tree, the game's error code }, read behind the work
 * `stream` holds and waiting for THAT stream only — agx_engine_game_info synchronises the whole device, which would also wait for a network
 * launch running beside the search on another stream. */
int agx_engine_root_summary(AgxEngine* engine, int game, void* stream, int* out4);
/* GeneratorThread::saveGames / loadGames (selfplay/GeneratorManager.cpp:98-122, GameGenerator::save / load, GameGenerator.cpp:122-141) for a
 * self-play pool: agx_engine_save_games lists the games in flight (h_out NULL: only counts them); agx_engine_restore_game, after
 * agx_engine_begin, makes pool slot game_slot continue from the saved position with an empty tree and solver table (GameGenerator::load calls
 * prepare_search on a fresh Tree) — the slot's game index starts again at 0 in the new pool. */
int agx_engine_save_games(AgxEngine* engine, AgxSavedGame* h_out, int capacity, int* count);
int agx_engine_restore_game(AgxEngine* engine, const AgxSavedGame* game, void* stream);
/* Search::solve(endTime >= 0) (search/monte_carlo/Search.cpp:159-183, called by SearchThread::asynchronous_run, player/SearchThread.cpp:150,168): the
 * solver's node limit becomes `max_nodes` (the reference: 10 000) and the leaves of the group's batches share `seconds` of wall-clock time from
 * the start of the launch — leaf i of a batch gets (time left) / (batch size - i), a leaf whose time is over stops after the node it is in
 * (AlphaBetaSearch.cpp:110-111,277).  seconds <= 0: every leaf gets its first node only.  Runs the serial solver (one wave per game) behind a
 * select stage enqueued separately (agx_engine_select_group); results depend on the clock, like the reference's. */
int agx_engine_solve_timed_group(AgxEngine* engine, int group, int n_groups, int max_nodes, double seconds, void* stream);
int agx_engine_set_force_expand_root(AgxEngine* engine, int force_expand_root); /* AgxEngineConfig.force_expand_root, for the launches that follow */
int agx_engine_buffers(AgxEngine* engine, AgxEngineBuffers* out);
int agx_engine_stats(AgxEngine* engine, AgxEngineStats* out);
/* Device memory this engine holds (every hipMalloc of agx_engine_create: tree heaps, the solver tables — 16 bytes x tss_table_entries per
 * game —, task / exchange buffers, the solver's spill areas and undo snapshots, record pools).  What one rank of a multi-GPU job needs of its
 * GPU's HBM next to the network's weights (GeneratorManager.cpp:146-152: one generator thread, i.e. one such pool, per device). */
int agx_engine_device_bytes(AgxEngine* engine, unsigned long long* bytes);
/* The same number for an engine that has not been created: what agx_engine_create(cfg) would allocate on a device with `compute_units` compute units
 * (256 on MI355X).  Touches no device — a launcher can size its ranks (one pool per device, GeneratorManager.cpp:146-152) before it starts them. */
int agx_engine_estimate_device_bytes(const AgxEngineConfig* cfg, int compute_units, unsigned long long* bytes);
/* Waves of the speculative search launch over the whole pool (AgxEngineConfig.speculative_waves, or the default resolved for this device, rules and
 * board); 0 when the pool runs the serial solver.  A group's launch takes waves / n_groups of them. */
int agx_engine_speculative_waves(AgxEngine* engine, int* waves);
/* Per-kernel timing of the engine's own launches, by HIP events recorded on the launch stream around every kernel (the role of
 * SearchStats' TimedStat members, search/monte_carlo/Search.hpp, for the device kernels).  Synchronises the device, returns the
 * time and launch count accumulated since the previous call in ms_out[4] / launches_out[4] (0 k_select, 1 k_solve, 2 k_expand,
 * 3 k_advance; either pointer may be null), then switches recording on or off. */
int agx_engine_kernel_timing(AgxEngine* engine, int enable, double* ms_out, long long* launches_out);
/* Tree::getInfo({}) of one game (Tree.cpp:403-424): root snapshot + board. */
int agx_engine_game_info(AgxEngine* engine, int game, AgxGameInfo* info, uint8_t* h_board, AgxEdgeView* h_root_edges, int edge_capacity);
/* Tree::getInfo(moves) for any move path (Tree.cpp:403-424) and the principal variation built on it (player/SearchEngine.cpp:219-230,243-266),
 * read from the device tree without changing it.  A path starts at the tree's base board (the position of the last set-board or played move)
 * and puts its moves on with alternating colours, the first one of the side to move; only the row and column of a Move::toShort are read.
 * The position reached is sought in the tree's node cache.  An occupied cell or a position that is not cached gives found = 0 (the
 * reference's empty Node()), not an error; a row or column outside the board is AGX_ERR_INVALID.  `game` is the pool slot (match mode: that
 * player's tree); a tournament-search engine has one tree, game 0.  Both calls run one launch behind the work `stream` holds and wait for THAT
 * stream only; call them between two steps of the tree. */
typedef struct AgxNodeView
{ /* ag::Node (Node.hpp:24-42) of the position a path leads to */
	int found;          /* 0: occupied cell on the path, or the position is not cached (every other field 0) */
	int visits;
	float win, draw, moves_left;
	int score;          /* Score raw bits */
	int flags;          /* root 2, fully expanded 4, statically solved 8, recursively solved 16, must defend 32 */
	int sign_to_move, depth, virtual_loss;
	int n_edges;        /* the node's full edge count, also when fewer edges were copied */
} AgxNodeView;
/* n_paths paths in one launch, one wave per path: path i is h_moves[h_path_offsets[i] .. h_path_offsets[i + 1]) (n_paths + 1 offsets).
 * h_nodes[i] receives its node, h_edges[i * edges_per_path ..] the first min(n_edges, edges_per_path) of its edges (h_edges may be NULL
 * with edges_per_path 0). */
int agx_engine_node_info(AgxEngine* engine, int game, const uint16_t* h_moves, const int* h_path_offsets, int n_paths,
		AgxNodeView* h_nodes, AgxEdgeView* h_edges, int edges_per_path, void* stream);
/* The principal variation from the end of the path h_moves[0 .. n_moves) in one launch: while the node is cached and has edges, the edge of
 * BestEdgeSelector (EdgeSelector.cpp:515-536, the "best" final selector: first strict maximum) is taken and its child sought, for at most
 * max_length plies.  *length receives the number of plies; h_pv[k] the move (Move::toShort) and h_pv_edges[k] the edge chosen at ply k;
 * h_pv_nodes[k] (max_length + 1 entries) the node of the position after k plies, the last one the node the walk stopped at.  h_pv_edges and
 * h_pv_nodes may be NULL. */
int agx_engine_principal_variation(AgxEngine* engine, int game, const uint16_t* h_moves, int n_moves, int max_length,
		uint16_t* h_pv, AgxEdgeView* h_pv_edges, AgxNodeView* h_pv_nodes, int* length, void* stream);
int agx_engine_records(AgxEngine* engine, AgxMoveRecord* h_records, int record_capacity, AgxEdgeView* h_edges, int edge_capacity, int* n_records, int* n_edges);
/* Same, then empties the device-side record pools (what GeneratorManager::addToBuffer's hand-over does, GeneratorManager.cpp:
 * 160-164): a long-running loop calls this every few hundred steps so that record_capacity is never exhausted. */
int agx_engine_drain_records(AgxEngine* engine, AgxMoveRecord* h_records, int record_capacity, AgxEdgeView* h_edges, int edge_capacity, int* n_records, int* n_edges);
/* Everything the record pools hold: move records, root-edge snapshots (record_format bit 0), format-201 sample bytes (bit 1) and
 * finished games.  Any buffer may be NULL (with capacity 0) to skip that part; `counts` receives what the device holds.  drain != 0
 * empties all four pools afterwards (GeneratorManager::addToBuffer's hand-over, GeneratorManager.cpp:160-164). */
int agx_engine_fetch_records(AgxEngine* engine, AgxMoveRecord* h_records, int record_capacity, AgxEdgeView* h_edges, int edge_capacity,
		uint8_t* h_samples, int sample_capacity, AgxGameEnd* h_game_ends, int game_end_capacity, AgxRecordCounts* counts, int drain);
/* Match mode, the efficient way to step: every stage is ONE launch over both players' trees (about half of them search at any time),
 * only the network stage runs per player: select/solve for all, first_net on the first players' leaves, second_net on the second
 * players', expand/backup/move for all.  A tree that gets the move in this step starts searching in the next one; per-tree
 * results are the same as with two agx_engine_step_group calls (each tree performs the same sequence of operations). */
int agx_engine_step_match(AgxEngine* engine, AgxNet* first_net, AgxNet* second_net, void* stream);
int agx_engine_select_solve_match(AgxEngine* engine, void* stream);  /* the stages separately: this, then                        */
int agx_engine_expand_backup_match(AgxEngine* engine, void* stream); /* agx_engine_evaluate_group(e, net, 0 / 1, 2, s), then this */
/* Match mode: h_results int[n_games / 2][4] = games won / drawn / lost by the FIRST player of each pair and the games the pair has
 * finished (what EvaluationManager sums per player, evaluation/EvaluationManager.cpp); the moves of every game are in the records. */
int agx_engine_match_results(AgxEngine* engine, int* h_results, int pair_capacity);
/* The same totals over all pairs, added up on the device by one small launch behind the work `stream` holds: out[0..2] = games won / drawn /
 * lost by the first player, out[3] = games finished.  Waits for THAT stream only and copies 32 bytes — what a loop that polls "are all
 * games played?" wants instead of agx_engine_match_results' device-wide synchronise and its copy of every pair's record. */
int agx_engine_match_summary(AgxEngine* engine, long long out[4], void* stream);
/* Match mode: PAIR RESULTS, logged on the device.  A pair result is what the first player took from one opening played twice with the
 * colours swapped: 2 points per win, 1 per draw, 0..4 (the reference's get_points / convert_match_results) — what a sequential test
 * (GSPRT) consumes one at a time in a fixed order, and what the running totals above cannot give back once two openings of a pair have
 * been added up.  agx_engine_match_track_pairs switches the log on: `capacity` entries, allocated once and freed with the engine.  From
 * then on ONE 256-thread workgroup follows every advance launch of the pool (merged: agx_engine_expand_backup_match / agx_engine_step_match;
 * group-stepped: the advance stage of either group) on that launch's stream and appends an entry for every pair that has finished an
 * opening since its previous entry.  The log's order is launch, then pair index: it does not depend on how the device schedules the
 * games, so two runs of the same pool log the same sequence.  (The advance stages of a pool are issued in stream order, as they already must be:
 * the log has one writer at a time.)  A pool that never calls agx_engine_match_track_pairs launches exactly what it did before.
 *   status: AGX_ERR_STATE on a pool without match_mode, after agx_engine_begin, and for a second call; AGX_ERR_INVALID for capacity < 1.
 * agx_engine_begin empties the log and zeroes the totals.
 * agx_engine_match_pair_results copies entries first .. min(logged, first + capacity) to h_out and the totals to totals[8], behind the work
 * `stream` holds (it waits for that stream only); h_out may be NULL with capacity 0: the totals alone.  logged = min(totals[5], the log's
 * capacity), so the call has written max(0, min(logged, first + capacity) - first) entries.
 *   totals[0..4] histogram of the points; [5] results seen, logged or not; [6] flags: 1 the log was full (the result is counted in [0..5]
 *   and not written), 2 a pair finished more than one opening between two log launches, 4 a pair's scores did not add up to two games (2 and
 *   4 cannot happen with the stepping calls above; such a pair is neither logged nor counted, and its next opening is read afresh);
 *   [7] log launches since agx_engine_begin.
 *   status: AGX_ERR_STATE before agx_engine_begin, on a pool without match_mode or without tracking; AGX_ERR_INVALID for null totals, a
 *   negative first or capacity, a NULL h_out with capacity > 0. */
typedef struct AgxPairResult
{
	int32_t pair;   /* the pair (= the first player's tree) */
	int32_t round;  /* the pair's games_done / 2 - 1: its opening was number pair + round * (n_games / 2) of the pool's list */
	int32_t points; /* 0..4, the first player's */
	int32_t launch; /* the log launch that found it, counted from 0 at agx_engine_begin */
} AgxPairResult;
int agx_engine_match_track_pairs(AgxEngine* engine, int capacity);
int agx_engine_match_pair_results(AgxEngine* engine, int first, AgxPairResult* h_out, int capacity, long long totals[8], void* stream);
/* Match mode: each player with search settings of its own.  The reference hands every player of an evaluation game a SelfplayConfig
 * (EvaluationGame::setFirstPlayer / setSecondPlayer; evaluation/Player.cpp:64-81 takes search_config, final_selector,
 * constraints.max_simulations and max_batch_size from it), which is how tuning_launcher plays a base configuration against a tested one on
 * one network.  Both players of a pool start with the pool's AgxEngineConfig; agx_engine_set_player_search replaces one player's settings
 * from the next stage launch on (call it between two steps), agx_engine_player_search reports what a player searches with now.  player 0 is
 * the first player (trees 0 .. n_games/2 - 1), player 1 the second.  agx_engine_set_max_simulations / agx_engine_set_batch_size keep their
 * meaning: they set that field for BOTH players; the last call wins.  Root noise, use_symmetries and the seeds, the table and arena sizes,
 * draw_after, the yield / speculative settings and the pruned root stay the pool's.
 * Status: AGX_ERR_STATE on a pool without match_mode; AGX_ERR_INVALID (agx_last_error names the field and its range) for a null argument, a
 * player other than 0 / 1 and a field outside the range given below — the call then changes nothing. */
typedef struct AgxPlayerSearch
{
	int max_simulations;              /* Constraints::max_simulations of this player, >= 50 (see AgxEngineConfig.max_simulations).  NB the pool and
	                                     agx_engine_set_max_simulations only ADVISE >= 50 and accept any positive value: a player they left below
	                                     50 is reported as it is, and a set call for that player must raise max_simulations to >= 50 too */
	int max_batch_size;               /* Search::setBatchSize: 1 .. the pool's max_batch_size (the task buffers keep the pool's stride) */
	float exploration_constant;
	float exploration_scaling;
	int init_to;                      /* 0..3 as AgxEngineConfig */
	float information_leak_threshold;
	int max_children;                 /* 0 = unlimited */
	float policy_expansion_threshold;
	float policy_temperature;         /* >= 0 */
	int tss_max_positions;            /* 1 .. the pool's tss_max_positions (allocations and the speculative decision stay the pool's) */
	int final_selector;               /* 0..5 as AgxEngineConfig */
	int action_values;                /* 0: this player's network is a 'pv' network, its new edges start at (0, 0); 1: a 'pvq' network — only in a
	                                     pool created with action_values = 1 (the action-values exchange buffer exists).  agx_engine_evaluate_group /
	                                     agx_engine_step_match run the 'pvq' forward for a player that asks for it and refuse a network without the
	                                     head for that player only: a 'pv' generation can be gated against the 'pvq' one that replaces it. */
} AgxPlayerSearch;
int agx_engine_player_search(AgxEngine* engine, int player, AgxPlayerSearch* out);
int agx_engine_set_player_search(AgxEngine* engine, int player, const AgxPlayerSearch* in);
/* Appends openings to the pool's list.  Finished games take the next unused opening in game order after every step; games that
 * found none left wait and pick one up here (the reference's generators produce openings on demand, GameGenerator.cpp:54-77). */
int agx_engine_add_openings(AgxEngine* engine, const uint16_t* h_openings, int n_openings);
/* FastZobristHashing keys used by the solver tables: uint64[2 * cells][2] = (lo, hi) per (cell, colour). */
int agx_engine_zobrist(AgxEngine* engine, uint64_t* h_keys, size_t n_words);

/* Test hooks: run single stages on caller-supplied positions (boards uint8[count][cells], 0 empty 1 cross 2 circle). */
int agx_debug_solve(AgxEngine* engine, const uint8_t* h_boards, const int* h_signs, int count, uint32_t* h_features, uint16_t* h_moves,
		uint16_t* h_scores, int* h_counts, uint32_t* h_flags, uint16_t* h_result_scores);
int agx_debug_solve_nodes(AgxEngine* engine, int count, unsigned long long* h_nodes);   /* solver nodes visited per position by the last agx_debug_solve (AlphaBetaSearch::solve's return value) */
int agx_debug_new_generation(AgxEngine* engine);                                       /* AlphaBetaSearch::increaseGeneration for the positions agx_debug_solve solves */
int agx_debug_pattern_state(AgxEngine* engine, const uint8_t* h_boards, const int* h_signs, const uint16_t* h_moves, int count, int n_moves,
		uint8_t* h_ptypes, uint8_t* h_threats, int16_t* h_lists, int lists_stride);
/* Host-only: the lookup tables the engine uploads (pattern uint8[1<<20], half-open-three uint8[1<<20], threat uint8[4096][2],
 * defence uint16[15][256][2]) for verification against the reference tables. */
int agx_host_tables(int rules, uint8_t* h_pattern, uint8_t* h_half_open_three, uint8_t* h_threat, uint16_t* h_defense);

/* ------------------------------------------------------------------------------------------------
 * Self-play record sink: finished games in the reference's dataset format 201.
 * Replaces GameDataStorage / GameDataBuffer on the producing side (src/dataset/GameDataStorage.cpp:217-250,
 * src/dataset/GameDataBuffer.cpp:97-113) and GeneratorManager::addToBuffer (src/selfplay/GeneratorManager.cpp:160-164).
 * The samples themselves are quantised on the device (AgxEngineConfig.record_format bit 1).
 * ---------------------------------------------------------------------------------------------- */
typedef struct AgxGameBuffer AgxGameBuffer; /* opaque; every call locks the buffer's mutex, so one buffer may serve the generator threads of several GPUs */

typedef struct AgxGameBufferStats
{ /* GameDataBufferStats (dataset/GameDataBuffer.hpp) */
	int games, samples, cross_win, draws, circle_win, game_length;
} AgxGameBufferStats;

int agx_game_buffer_create(int rules, int rows, int cols, int draw_after, AgxGameBuffer** out);
int agx_game_buffer_destroy(AgxGameBuffer* buffer);
int agx_game_buffer_clear(AgxGameBuffer* buffer);
/* Drains the engine's record pools (synchronises its device) and appends every game that has finished: samples by move number, all
 * moves of the game, outcome, rows, cols = the bytes of GameDataStorage::serialize.  Samples of games still running are kept until
 * their game ends.  The engine must record format-201 samples.  games_added may be NULL. */
int agx_game_buffer_collect(AgxGameBuffer* buffer, AgxEngine* engine, int* games_added);
int agx_game_buffer_stats(const AgxGameBuffer* buffer, AgxGameBufferStats* out);
/* GameDataStorage::serialize bytes of game `index`; h_bytes == NULL only queries *size. */
int agx_game_buffer_game(const AgxGameBuffer* buffer, int index, uint8_t* h_bytes, size_t capacity, size_t* size);
/* GameDataBuffer::save: {"format": 201, "config": {...}, "offsets": [...]} + newline + the games' bytes; compress != 0 wraps the file in
 * a zlib stream (the reference compresses with MinML's ZipWrapper, whose format is not in the reference tree). */
int agx_game_buffer_save(const AgxGameBuffer* buffer, const char* path, int compress);
/* GameDataBuffer::load (dataset/GameDataBuffer.cpp:115-131; called by GeneratorManager::loadState, GeneratorManager.cpp:263-275) for files written
 * by agx_game_buffer_save, compressed or not: the games are appended to the buffer */
int agx_game_buffer_load(AgxGameBuffer* buffer, const char* path);
/* the game configuration in the header of such a file */
int agx_game_buffer_file_config(const char* path, int* rules, int* rows, int* cols);
/* Checkpoints of games in flight (GameGenerator::save / load, selfplay/GameGenerator.cpp:122-141): the format-201 samples a game has collected
 * so far wait in the buffer, keyed by (engine, game_slot, game_index), until its AgxGameEnd arrives.  take_pending serialises and removes
 * them ({ i32 move number, u32 bytes, sample } records; h_bytes NULL: size only, nothing removed); restore_pending hands them to the game that
 * continues it in another engine (agx_engine_restore_game: game_index 0); forget_engine drops whatever an engine that is about to be destroyed
 * left pending. */
int agx_game_buffer_take_pending(AgxGameBuffer* buffer, const AgxEngine* engine, int game_slot, int game_index, uint8_t* h_bytes, size_t capacity, size_t* size);
int agx_game_buffer_restore_pending(AgxGameBuffer* buffer, const AgxEngine* engine, int game_slot, int game_index, const uint8_t* h_bytes, size_t size);
int agx_game_buffer_forget_engine(AgxGameBuffer* buffer, const AgxEngine* engine);
/* the game configuration the buffer was created for; any output may be NULL */
int agx_game_buffer_config(const AgxGameBuffer* buffer, int* rules, int* rows, int* cols, int* draw_after);
/* Host-only reader of one format-201 sample (SearchDataStorage_v201's parsing constructor + storeTo, dataset/SearchDataStorage.cpp:
 * 300-320,375-409): per cell visits int32[rows*cols], prior float[rows*cols], value float[rows*cols][2] = (win, draw), score
 * uint16[rows*cols]; header int[3] = (minimax score raw bits, move number, flags); minimax_value float[2].  consumed may be NULL. */
int agx_sample_v201_unpack(const uint8_t* h_bytes, size_t size, int rows, int cols, int32_t* visits, float* prior, float* value, uint16_t* score,
		int* header, float* minimax_value, size_t* consumed);

/* ----------------------------------------------------------------------------------------------
 * Training batches: format-201 games -> network tensors, on the device (csrc/training_batch.hip).
 * What the reference's dataset reader does on one host thread (src/dataset/torch_api.cpp: load_dataset_fragment, get_dataset_size,
 * get_tensor_shapes, load_batch): per sample the board is rebuilt from the game's moves, the sample dequantised
 * (SearchDataStorage_v201::storeTo), one of the 8 symmetries applied, the input features encoded (PatternCalculator::setBoard +
 * NNInputFeatures::encode) and the training targets written.  Here one wavefront does that per sample, a whole batch in one launch.
 * A dataset holds numbered fragments of one game configuration (square boards up to 20x20).  Everything except the two load_batch
 * calls is host work and needs no GPU: the games' bytes are uploaded at the first load_batch that uses their fragment.
 * ---------------------------------------------------------------------------------------------- */
typedef struct AgxDataset AgxDataset; /* opaque; every call locks the dataset's mutex */

typedef struct AgxDatasetSample
{ /* Sample_t (dataset/torch_api.h) */
	int fragment, game, sample, augmentation; /* augmentation: symmetry 0..7 (utils/augmentations.hpp) */
} AgxDatasetSample;

typedef struct AgxTensorShape
{ /* TensorSize_t (dataset/torch_api.h) */
	int rank, dim[4];
} AgxTensorShape;

enum
{
	AGX_BATCH_INPUT_FP16 = 1,    /* d_input holds IEEE half values instead of float32 */
	AGX_BATCH_POLICY_VISITS = 2, /* policy target of SamplerVisits (dataset/Sampler.cpp:96-133): a proven draw keeps its visit count; default: torch_api.cpp's max(1, visits) */
	AGX_BATCH_POLICY_VALUES = 4  /* policy and action-value targets of SamplerValues (dataset/Sampler.cpp:138-214), the reference's default sampler; not together with AGX_BATCH_POLICY_VISITS */
};

int agx_dataset_create(int rules, int rows, int cols, AgxDataset** out);
int agx_dataset_destroy(AgxDataset* dataset);
/* Fragment `fragment` (any number >= 0 that is not loaded yet) from a file written by agx_game_buffer_save (compressed or not), or a copy of
 * the finished games of a live buffer.  AGX_ERR_INVALID with a message in agx_last_error() when the rules or the board differ from the
 * dataset's, when a game's bytes do not follow the format-201 layout, or when a sample points outside its game or its board. */
int agx_dataset_add_fragment_file(AgxDataset* dataset, int fragment, const char* path);
int agx_dataset_add_fragment_buffer(AgxDataset* dataset, int fragment, const AgxGameBuffer* buffer);
int agx_dataset_unload_fragment(AgxDataset* dataset, int fragment); /* waits for the batches of this dataset that are still in flight */
int agx_dataset_games(const AgxDataset* dataset, int* games);
/* get_dataset_size: per game, fragments in ascending order, (fragment, game, samples, symmetries) */
int agx_dataset_sizes(const AgxDataset* dataset, int* h_sizes, int capacity_games);
int agx_dataset_stats(const AgxDataset* dataset, AgxGameBufferStats* out); /* sums over all fragments */
/* get_tensor_shapes for a batch of n samples; any output may be NULL.  input [n, rows, cols, 32], features [n, rows * cols],
 * policy [n, rows, cols], value [n, 3], moves_left [n, 1], action_values [n, rows, cols, 3] */
int agx_dataset_tensor_shapes(const AgxDataset* dataset, int n, AgxTensorShape* input, AgxTensorShape* features, AgxTensorShape* policy_target,
		AgxTensorShape* value_target, AgxTensorShape* moves_left_target, AgxTensorShape* action_values_target);
/* One launch on `stream` writes sample b of h_samples to index b of every output (device addresses, each aligned to its element type):
 *   d_input          [n][rows][cols][32] bit j of the feature word as 0 / 1, float32 or (AGX_BATCH_INPUT_FP16) half; may be NULL
 *   d_features       [n][rows * cols] the feature words themselves, the form agx_nn_forward takes; may be NULL
 *   d_policy         [n][rows][cols] float32, sums to 1 (float32 sum in cell order of the transformed board, then * 1.0f / sum)
 *   d_value          [n][3] (win, draw, loss) of the game's outcome for the side to move
 *   d_moves_left     [n][1]
 *   d_action_values  [n][rows][cols][3] (win, draw, loss) per cell — sample b at index b (see training_batch.hip on the reference here)
 * The call returns when the launch is enqueued; h_samples may be reused at once.  In the steady state it waits for nothing on the
 * device and synchronises nothing; on the host it may wait for the batch enqueued four calls earlier (whose record buffer it takes
 * over).  Three things allocate device memory and may therefore be serialised with the device's work by the runtime: the dataset's
 * first batch (tables, spill areas), the first batch that uses a fragment (its bytes are uploaded with a blocking copy) and a batch
 * larger than any of the four before it in its record slot (at least 1024 samples fit from the start).  The dataset lives on the HIP
 * device that is current at its first batch: AGX_ERR_STATE when a later call finds another one current.
 * A fragment, game, sample or augmentation out of range is AGX_ERR_INVALID before anything is launched.  Under renju the foul test
 * follows nested 3x3 forks 16 deep; a sample beyond that (no known game has one) gets features that are not to be trusted: the
 * host-pointer form returns AGX_ERR_STATE for its batch, this form at the next call on the dataset, naming the sample. */
int agx_dataset_load_batch(AgxDataset* dataset, int n, const AgxDatasetSample* h_samples, void* d_input, uint32_t* d_features, float* d_policy,
		float* d_value, float* d_moves_left, float* d_action_values, int flags, void* stream);
/* the same into host memory (the dataset owns the device staging and a stream of its own; one launch, one copy back per output, returns
 * when the data is there).  Calls from several threads run one after the other. */
int agx_dataset_load_batch_host(AgxDataset* dataset, int n, const AgxDatasetSample* h_samples, void* h_input, uint32_t* h_features, float* h_policy,
		float* h_value, float* h_moves_left, float* h_action_values, int flags);
/* The extended form: the same launch with one more output, and the form new outputs will be added to.  The two calls above forward to it
 * with action_values_weight = NULL and write exactly what they wrote before it existed.
 *   action_values_weight [n][rows][cols] float32, may be NULL: the weight of the cell in the action-value loss, visits / sum of visits as
 *                    the reference's fill_action_values_mask forms it (selfplay/SupervisedLearning.cpp:55-61): w = float(c) * (1.0f /
 *                    float(sum of c)), with c = max(1, visits) on an empty cell with a proven score and c = visits on every other cell — the
 *                    count both of the reference's samplers leave in TrainingDataPack::visit_count.  The same in every policy mode.  When
 *                    the sum is 0 every weight is 0.0f (this project's rule: the reference would divide by zero).
 * AGX_BATCH_POLICY_VALUES (not together with AGX_BATCH_POLICY_VISITS: AGX_ERR_INVALID before anything is launched) writes what
 * SamplerValues::prepare_training_data (dataset/Sampler.cpp:138-214) writes, in float32, one operation after the other, unfused.  With
 * board = the transformed board, prior = PriorFormat::decode * policy_scale, q(cell) = the expectation win + 0.5f * draw of the proven
 * score's value or else of the stored action value, V = the same of the sample's minimax value and score (storeTo's rule, its sums taken
 * in entry order), and `counted` = an empty cell with visits > 0 or a proven score:
 *   sum_P, sum_PxQ   prior and prior * q added over the counted cells in cell order, from 0.0f; u = the number of the other empty cells
 *   base             = sum_P * sum_PxQ + (1.0f - sum_P) * V
 *   logit            = 50.0f * Q + logf(FLT_EPSILON + P) on every empty cell: Q = base, P = max(0.0f, (1.0f - sum_P) / u) on a cell that is
 *                      not counted (u == 0: there is no such cell, nothing is divided); on a counted cell P = prior and Q = -1.0f / (1.0f +
 *                      distance) for a proven loss, 0.5f for a proven draw, 1.0f + 2.0f / (1.0f + distance) for a proven win, the stored
 *                      action value's expectation otherwise
 *   policy           = e / sum on the empty cells (a true division), e = expf(max(-20.0f, logit - the largest logit)), sum = the e added
 *                      in cell order from 0.0f; exactly 0.0f on occupied cells
 *   action values    as in the other modes on the counted cells, (0, 0, 1) on every other cell
 * All sums run in cell order of the TRANSFORMED board (the reference samples first and applies the symmetry afterwards: its sums run in
 * the untransformed order; the two differ by float32 rounding only).  logf and expf are the device's: within 1 ulp of a host libm. */
typedef struct AgxBatchTensors
{ /* device addresses for agx_dataset_load_batch_ex, host addresses for agx_dataset_load_batch_host_ex */
	void* input;                 /* may be NULL */
	uint32_t* features;          /* may be NULL */
	float* policy;
	float* value;
	float* moves_left;
	float* action_values;
	float* action_values_weight; /* may be NULL */
} AgxBatchTensors;
int agx_dataset_load_batch_ex(AgxDataset* dataset, int n, const AgxDatasetSample* h_samples, const AgxBatchTensors* tensors, int flags, void* stream);
int agx_dataset_load_batch_host_ex(AgxDataset* dataset, int n, const AgxDatasetSample* h_samples, const AgxBatchTensors* tensors, int flags);

/* ----------------------------------------------------------------------------------------------
 * Scoring a network against saved games: losses and top-k accuracy, on the device (csrc/net_score.hip).
 * The step a training loop runs between "new checkpoint" and "hand it to the self-play pool" (the reference: SupervisedLearning::validate
 * with AGNetwork::getLoss and getAccuracy).  getAccuracy (src/networks/NetworkDataPack.cpp:321-345) is followed literally; MinML's loss
 * code is not in the reference tree, so the loss formulas below are this project's own.  Per sample, with the network's outputs in the
 * layout agx_nn_forward[_pvq] writes and the targets in the layout agx_dataset_load_batch writes:
 *   policy_ce  = - sum over the cells with target t > 0 of t * log(max(p, FLT_MIN))
 *   value_ce   = the same sum over the 3 value outputs
 *   q_ce       = - sum of t_c * log(max(q_c, FLT_MIN)) over the 3 classes (win, draw, loss) of every cell whose POLICY target is > 0 (the
 *                cells that had an edge: the other cells' action-value targets are filler); the output's loss class is the float32
 *                1.0f - win - draw; q_cells counts those cells.  Both 0 without action values.
 *   topk_hit   = getAccuracy with top_k = 4: correct = the first maximum of the policy target in row-major order (pickMove, utils/misc.cpp:
 *                79-83); four times: best = the first maximum of the outputs, topk_hit[l..3] += 1 when best == correct, then the output at
 *                best becomes 0 (in a copy: the caller's buffer is only read).  Once only zeros are left `best` stays on cell 0, so a sample
 *                whose correct move is cell 0 can count more than once, as in the reference.  (std::max_element's way with NaNs is kept
 *                too: a NaN on cell 0 is the maximum, any other NaN never is.)
 * Every term is a float32 product of the float32 target and logf; a sample's terms are summed in float64 in a fixed order, the samples in
 * sample order: totals are bit-identical however a set of samples is split into calls and wherever the launches run.
 * ---------------------------------------------------------------------------------------------- */
typedef struct AgxSampleScore
{ /* 48 bytes */
	double policy_ce, value_ce, q_ce;
	int32_t q_cells;
	int32_t topk_hit[4];
	int32_t reserved; /* written as 0 */
} AgxSampleScore;

typedef struct AgxNetScore
{ /* 72 bytes; sums over `samples` samples */
	int64_t samples;
	double policy_ce, value_ce, q_ce;
	int64_t q_cells;
	int64_t topk_hit[4];
} AgxNetScore;

/* Zeroes *d_total on `stream`. */
int agx_net_score_clear(AgxNetScore* d_total, void* stream);
/* Scores n samples and ADDS them to *d_total (device memory the caller has cleared or chained from earlier calls).  All pointers are device
 * addresses: d_policy float[n][rows*cols], d_value float[n][3], d_action_values float[n][rows*cols][2] or NULL; d_policy_target
 * float[n][rows*cols], d_value_target float[n][3], d_action_values_target float[n][rows*cols][3] (NULL exactly when d_action_values is).
 * Two launches on `stream`, nothing else, nothing synchronised: one wavefront per sample writes d_sample_scores[n], one workgroup adds
 * them up in sample order.  d_sample_scores == NULL is a CONVENIENCE PATH for callers with a few samples and no use for the records: they
 * stay on the chip, in ONE launch of one workgroup that scores 16 samples at a time (the same bits, but a single compute unit does all the
 * work: pass a records buffer for anything large, as agx_net_score_dataset does).  Boards 5..20 x 5..20. */
int agx_net_score_outputs(int rows, int cols, int n, const float* d_policy, const float* d_value, const float* d_action_values,
		const float* d_policy_target, const float* d_value_target, const float* d_action_values_target, AgxSampleScore* d_sample_scores,
		AgxNetScore* d_total, void* stream);
/* The whole path for n samples of a dataset, `chunk` at a time (0 = 1024): agx_dataset_load_batch (feature words and targets),
 * agx_nn_forward or agx_nn_forward_pvq according to the network's description, agx_net_score_outputs — all on `stream`, in device
 * scratch the call allocates for one chunk and frees before it returns; one 72-byte copy back into *h_out at the end (the call waits for
 * it).  The total does not depend on `chunk`.  AGX_ERR_INVALID: null arguments, n <= 0, negative chunk, a dataset whose board is not the
 * network's; the dataset's and the network's own errors pass through. */
int agx_net_score_dataset(AgxNet* net, AgxDataset* dataset, int n, const AgxDatasetSample* h_samples, int chunk, AgxNetScore* h_out, void* stream);
/* agx_net_score_outputs with a weight per cell for the action-value term: d_q_weight float[n][rows*cols], the action_values_weight of
 * agx_dataset_load_batch_ex (needs the two action-value tensors).  A cell then counts when its weight is > 0, not when its policy target
 * is: its three float32 terms are added in class order in float64 from 0.0, the sum is multiplied by (double) w and added to q_ce;
 * q_cells counts the cells with w > 0.  A cell whose weight is not > 0 (zero, negative, NaN) is not read: a NaN among its outputs or
 * targets reaches nothing.  q_ce / samples is then the mean of the per-sample weighted means, the loss the reference's weight 0.05 of the
 * action-value output was chosen for.  d_q_weight == NULL gives the bits of agx_net_score_outputs.  Chaining and determinism as above. */
int agx_net_score_outputs_weighted(int rows, int cols, int n, const float* d_policy, const float* d_value, const float* d_action_values,
		const float* d_policy_target, const float* d_value_target, const float* d_action_values_target, const float* d_q_weight,
		AgxSampleScore* d_sample_scores, AgxNetScore* d_total, void* stream);
/* agx_net_score_dataset with the loader's flags (AGX_BATCH_POLICY_VISITS or AGX_BATCH_POLICY_VALUES; AGX_BATCH_INPUT_FP16 is refused: the
 * path reads feature words, no input planes) and, with q_weighted != 0, the weighted action-value term on the loader's
 * action_values_weight.  agx_net_score_dataset is this call with 0, 0. */
int agx_net_score_dataset_ex(AgxNet* net, AgxDataset* dataset, int n, const AgxDatasetSample* h_samples, int chunk, int batch_flags, int q_weighted,
		AgxNetScore* h_out, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Training: the loss of the three heads and its gradients with respect to the LOGITS, on the device (csrc/head_loss.hip).
 * The last layer of a training step: a torch module (alphagomoku_amd/training.py: TowerModule) produces pre-softmax outputs from the tensors
 * agx_dataset_load_batch writes, this call turns them into the losses agx_net_score_* reports and into dL/dlogits, torch's autograd and
 * optimiser do the rest.  The reference trains with MinML's graph (networks.cpp:89 graph.setOptimizer(ml::RAdam())); its loss code is not
 * in the reference tree, so the formulas are this project's own: the cross-entropies above in their log-sum-exp form.  Per sample and head
 * (policy over the board's cells, value over its 3 outputs, action values over the 3 classes of every cell on its own), with logits z:
 *   m = max z;  e_i = expf(z_i - m);  S = sum of e_i in float64 (per lane in cell order, then a fixed butterfly);  lse = m + logf((float) S)
 *   loss       = sum over the entries with target t > 0 of the float32 product t * (lse - z_i), added in float64.  A probability that
 *                underflows costs t * (lse - z), where agx_net_score_outputs floors it at FLT_MIN.
 *   gradient_i = scale * (p_i * T - t_i) with p_i = e_i / (float) S, T = the float32 of the float64 sum of the positive targets, and t_i
 *                counted as 0 unless it is > 0.  Written for EVERY element: the buffers need no clearing.
 *   q_ce, q_cells, d_q_grad: only the cells whose POLICY target is > 0 count (the mask of agx_net_score_outputs); on every other cell the
 *                gradient is exactly 0.0f and neither its logits nor its targets are read — the targets there are filler, a NaN among them
 *                reaches neither a loss nor a gradient.
 * Non-finite logits propagate, nothing is clamped.  d_sample_scores[n] receives the records (topk_hit and reserved written as 0), which
 * are added to *d_total in sample order by the reduction of agx_net_score_outputs: totals are bit-identical however a set of samples is
 * split into calls and wherever the launches run.  Two launches on `stream`, nothing synchronised.  d_q_logits / d_q_target: both or
 * neither; the gradients: one for every head that has logits, or all three NULL (losses only).  Boards 5..20 x 5..20.
 * AGX_ERR_INVALID before anything is launched otherwise. */
int agx_head_loss_grad(int rows, int cols, int n,
		const float* d_policy_logits,  /* [n][rows*cols], pre-softmax */
		const float* d_value_logits,   /* [n][3] */
		const float* d_q_logits,       /* [n][rows*cols][3] or NULL */
		const float* d_policy_target, const float* d_value_target,
		const float* d_q_target,       /* layouts of agx_dataset_load_batch; NULL exactly when d_q_logits is */
		float policy_scale, float value_scale, float q_scale,
		float* d_policy_grad, float* d_value_grad, float* d_q_grad,  /* same shapes as the logits; all three NULL = losses only */
		AgxSampleScore* d_sample_scores, /* [n], required */
		AgxNetScore* d_total,            /* added to, like agx_net_score_outputs */
		void* stream);
/* agx_head_loss_grad with a weight per cell for the action-value head: d_q_weight float[n][rows*cols], the action_values_weight of
 * agx_dataset_load_batch_ex (needs the action-value tensors).  A cell then counts when its weight w is > 0, not when its policy target is:
 *   q_ce       the cell's cross-entropy is formed as above (its float32 terms added in class order in float64, from 0.0), multiplied by
 *              (double) w and added to the sample's sum; q_cells counts the cells with w > 0
 *   gradient_i = (q_scale * w) * (p_i * T - t_i): the float32 product q_scale * w first, then its float32 product with the float32
 *              difference; with w == 1.0f these are the bits of the unweighted form
 * A cell whose weight is not > 0 (zero, negative, NaN) gets the gradient exactly 0.0f; neither its logits nor its targets are read, a NaN
 * among them or in the weight itself reaches nothing.  d_q_weight == NULL gives the bits of agx_head_loss_grad.  Chaining and determinism
 * as above: totals are bit-identical however a set of samples is split into calls. */
int agx_head_loss_grad_weighted(int rows, int cols, int n, const float* d_policy_logits, const float* d_value_logits, const float* d_q_logits,
		const float* d_policy_target, const float* d_value_target, const float* d_q_target, const float* d_q_weight, float policy_scale,
		float value_scale, float q_scale, float* d_policy_grad, float* d_value_grad, float* d_q_grad, AgxSampleScore* d_sample_scores,
		AgxNetScore* d_total, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Positions evaluated on the device: boards -> policy, value, best moves (csrc/position_eval.hip).
 * The primary entry point of the reference's network is AGNetwork::packInputData(index, board, signToMove) (AGNetwork.hpp:60), which encodes
 * the board on the host; agx_nn_forward takes feature words.  A position evaluator closes the gap for callers that hold boards and no
 * search: one launch encodes every (position, symmetry) row with the solver's own pattern code, the tower evaluates the rows, one launch
 * maps the rows back, averages them and picks the best legal cells.  Averaging over symmetries and the top-k are this project's own
 * (NNEvaluator draws one random symmetry per position).  With S = popcount(symmetry_mask), j the rank of symmetry s in the mask and T_s
 * the board under s (utils/augmentations.hpp):
 *   row p * S + j    = NNInputFeatures::encode(T_s(board p)), for every s in the mask in ascending order
 *   policy[p][c]     = (0.0f + row_s0[image_s0(c)] + row_s1[image_s1(c)] + ...) * (1.0f / S), float32, ascending s; image_s(c) is the cell
 *                      of T_s that shows cell c; then 0.0f on occupied cells and, with AGX_POSEVAL_MASK_FORBIDDEN, on the cells whose
 *                      identity-row feature word carries the renju forbidden bit (bit 6)
 *   value, action values: the same sum and multiplication (action values through image_s, not masked)
 *   AGX_POSEVAL_RENORMALISE: sum = the policy values added in cell order, one float32 addition after the other, from 0.0f; every value
 *                      is multiplied by 1.0f / sum; a sum of 0.0f leaves the values as they are (no NaN)
 *   top_k picks      k times: the largest policy value among the legal cells (empty and, with AGX_POSEVAL_MASK_FORBIDDEN, not
 *                      forbidden) not picked yet, of equal ones the lowest cell index (a NaN orders as -inf); cell -1 and probability
 *                      0.0f once no legal cell is left
 * Every output is a pure function of the tower's rows.  Boards of 15x15 and 20x20, all five rule sets.
 * ---------------------------------------------------------------------------------------------- */
typedef struct AgxPositionEvaluator AgxPositionEvaluator; /* opaque: pattern tables, the encode kernel's per-wave spill areas, and a features /
                                                             policy / value / action-values workspace of capacity x 8 rows; every call locks its mutex */

enum
{
	AGX_POSEVAL_MASK_FORBIDDEN = 1, /* policy 0.0f on renju fouls, which are then no legal cells either; needs symmetry 0 in the mask */
	AGX_POSEVAL_RENORMALISE = 2     /* the masked policy is scaled to sum 1 */
};
enum
{ /* status words */
	AGX_POSEVAL_STATUS_BAD_INPUT = 1,  /* a cell value above 2 or a sign other than 1 / 2: zero feature rows, zero outputs, cells -1 */
	AGX_POSEVAL_STATUS_FOUL_PROBE = 2  /* renju: 3x3 forks nest deeper than the foul test follows (16); the forbidden bits are not to be trusted */
};

typedef struct AgxPositionOutputs
{ /* device addresses; any of them may be NULL */
	float* policy;         /* [n][cells] */
	float* value;          /* [n][3] = (win, draw, loss) */
	float* action_values;  /* [n][cells][2] = (win, draw); 'pvq' networks only */
	int32_t* top_cells;    /* [n][top_k] row * board_size + col, or -1 */
	float* top_probs;      /* [n][top_k] */
	int32_t* status;       /* [n] 0 or AGX_POSEVAL_STATUS_* */
} AgxPositionOutputs;

/* Allocates everything the calls below use, on the current HIP device: they allocate nothing and synchronise nothing.  AGX_ERR_UNSUPPORTED for a
 * board size other than 15 or 20. */
int agx_position_evaluator_create(int rules, int board_size, int capacity, AgxPositionEvaluator** out);
int agx_position_evaluator_destroy(AgxPositionEvaluator* pe);
/* The encode launch alone, for callers that run the tower themselves: d_boards uint8[n][cells] (0 empty, 1 cross, 2 circle, what
 * agx_engine_set_board takes), d_signs uint8[n] (1 cross / 2 circle to move) -> d_features uint32[n * S][cells], d_status int32[n] (may be
 * NULL).  AGX_ERR_INVALID before anything is launched: n above the capacity, a mask of 0 or above 0xFF. */
int agx_position_evaluator_encode(AgxPositionEvaluator* pe, int n, const uint8_t* d_boards, const uint8_t* d_signs, int symmetry_mask,
		uint32_t* d_features, int32_t* d_status, void* stream);
/* The combine launch alone, on rows the caller got from the tower: d_policy_rows float[n * S][cells], d_value_rows float[n * S][3],
 * d_action_value_rows float[n * S][cells][2] (NULL unless out->action_values is set), d_features the encode launch's rows (read only with
 * AGX_POSEVAL_MASK_FORBIDDEN, else may be NULL), d_status_in its status words (may be NULL: every position counts as valid). */
int agx_position_evaluator_combine(AgxPositionEvaluator* pe, int n, const uint8_t* d_boards, int symmetry_mask, int flags, int top_k,
		const uint32_t* d_features, const float* d_policy_rows, const float* d_value_rows, const float* d_action_value_rows, const int32_t* d_status_in,
		const AgxPositionOutputs* out, void* stream);
/* Encode into the workspace, agx_nn_forward or (when out->action_values is set) agx_nn_forward_pvq on it, combine: three launches on
 * `stream`, nothing synchronised.  Refused before anything is launched — AGX_ERR_INVALID: n above the capacity, a mask of 0 or above 0xFF,
 * top_k outside 0..8, unknown flags, a network whose rows or cols differ from the evaluator's board, out->action_values with a network
 * that has no such head; AGX_ERR_UNSUPPORTED: AGX_POSEVAL_MASK_FORBIDDEN with a mask that leaves symmetry 0 out.  Calls on one evaluator
 * share its workspace: a call on another stream than the previous one is ordered behind it on the device. */
int agx_position_evaluator_evaluate(AgxPositionEvaluator* pe, AgxNet* net, int n, const uint8_t* d_boards, const uint8_t* d_signs, int symmetry_mask,
		int flags, int top_k, const AgxPositionOutputs* out, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Positions solved on the device: boards -> proven scores and the solver's action lists (k_solve_positions in csrc/engine.hip; the host side is csrc/position_solver.cpp).
 * The threat solver of the search (AlphaBetaSearch) for callers that hold boards: filtering provable samples out of a training set, puzzle
 * sets, opening checks, a move suggestion that respects forced defences.  Every position is solved as a fresh AlphaBetaSearch with an empty
 * table and node limit max_positions would solve it, so a position's result is a function of the position and of the arguments of
 * agx_position_solver_create alone — not of the batch, of the position's place in it, or of the number of waves.  One wavefront per
 * position; each wave owns a transposition table of table_entries entries (rounded up to a power of two, 16 bytes each), which it clears
 * before every position, and the solver's spill areas: agx_position_solver_info reports the waves and the bytes.  The wave count is
 * min(capacity, 4 per compute unit); the environment variable AGX_POSSOLVE_MAX_WAVES, read at create, caps it.  Square boards 5..20, all
 * five rule sets.
 * ---------------------------------------------------------------------------------------------- */
typedef struct AgxPositionSolver AgxPositionSolver;

enum
{ /* status words */
	AGX_POSSOLVE_STATUS_BAD_INPUT = 1,    /* a cell value above 2 or a sign other than 1 / 2: zeroed outputs, nothing reached the solver */
	AGX_POSSOLVE_STATUS_SOLVER_ERROR = 2  /* the solver gave up (the renju foul probe nested too deep, an action stack or frame overflow): outputs not to be trusted */
};

typedef struct AgxSolvedPositions
{ /* device addresses; any of them may be NULL */
	uint16_t* score;        /* [n] the 16-bit Score encoding of AgxEdgeView.score / agx_debug_solve's h_result_scores */
	uint32_t* flags;        /* [n] 1 must defend, 4 processed by the solver, 16 statically solved (at most one node), 32 recursively solved (proven) */
	int32_t* n_actions;     /* [n] */
	uint16_t* moves;        /* [n][cells] the solver's action list in the solver's ORDER (Move::toShort: sign | row << 2 | col << 9), zeros behind it */
	uint16_t* move_scores;  /* [n][cells] */
	uint32_t* nodes;        /* [n] AlphaBetaSearch::solve's return value */
	float* value;           /* [n][3] = (win, draw, loss) of a proven score (Score::convertToValue), zeros when unproven */
	int32_t* status;        /* [n] 0 or AGX_POSSOLVE_STATUS_* */
} AgxSolvedPositions;

/* Allocates everything agx_position_solver_solve uses, on the current HIP device.  AGX_ERR_UNSUPPORTED: board_size outside 5..20,
 * max_positions outside 1..1000; AGX_ERR_INVALID: a null argument, unknown rules, capacity outside 1..2^20, table_entries above 2^32 (below
 * that every value is taken, as by agx_engine_create: at least 4, rounded up to a power of two). */
int agx_position_solver_create(int rules, int board_size, int capacity, int max_positions, uint64_t table_entries, uint64_t zobrist_seed,
		AgxPositionSolver** out);
/* One launch on `stream`; nothing is allocated, nothing synchronised.  d_boards uint8[n][cells] (0 empty, 1 cross, 2 circle), d_signs
 * uint8[n] (1 cross / 2 circle to move).  AGX_ERR_INVALID before anything is launched: a null solver, `out`, boards or signs, n negative or
 * above the capacity.  Calls on one solver share its per-wave areas: a call on another stream than the previous one is ordered behind it on
 * the device. */
int agx_position_solver_solve(AgxPositionSolver* solver, int n, const uint8_t* d_boards, const uint8_t* d_signs, const AgxSolvedPositions* out,
		void* stream);
int agx_position_solver_destroy(AgxPositionSolver* solver);
/* waves of a launch, device bytes each wave owns (table, action stack, threat-list tails, frames, undo snapshots, task, game record,
 * feature words), and everything the solver allocated: waves x bytes_per_wave + the rule tables + the capacity-sized workspace of
 * agx_position_evaluator_evaluate_solved.  Any output may be NULL. */
int agx_position_solver_info(const AgxPositionSolver* solver, int* waves, uint64_t* bytes_per_wave, uint64_t* device_bytes);

/* The solver in front of the position evaluator: solve, encode, the tower, combine — four launches on `stream`, nothing synchronised.
 * `solved_out` (may be NULL, as may each of its members) receives what agx_position_solver_solve writes.  The tower runs on every row.
 * With L the solver's action list of a position:
 *   unproven score   policy as agx_position_evaluator_evaluate computes it, then 0.0f on every cell outside L (what the search does with a
 *                    task processed by the solver: the list is the move set, the network supplies the priors on it); then
 *                    AGX_POSEVAL_RENORMALISE by its rule; value: the network's
 *   proven score     value = the score's (win, draw, loss); policy = 1.0f / k on the k actions of L whose 16-bit score is the largest in L,
 *                    0.0f elsewhere (not renormalised, no mask applied); this split is the project's own definition
 *   top_k picks      by the rule of agx_position_evaluator_evaluate over that policy, among the cells of L that are legal there
 *   action values    the network's, unchanged
 *   status           the larger of the solver's and the evaluator's word; a position with bad input has zero outputs and cells -1
 * Refused before anything is launched: whatever agx_position_evaluator_evaluate refuses, a null solver, n above the solver's capacity,
 * and (AGX_ERR_INVALID) a solver whose rules or board size differ from the evaluator's. */
int agx_position_evaluator_evaluate_solved(AgxPositionEvaluator* pe, AgxPositionSolver* solver, AgxNet* net, int n, const uint8_t* d_boards,
		const uint8_t* d_signs, int symmetry_mask, int flags, int top_k, const AgxPositionOutputs* out, const AgxSolvedPositions* solved_out,
		void* stream);

/* ----------------------------------------------------------------------------------------------
 * Positions searched on the device: boards -> the root of a full search (PUCT, threat solver and network together, max_simulations
 * playouts per position; k_load_positions / k_harvest_positions in csrc/engine.hip; the host side is csrc/position_searcher.cpp).  Re-searching old samples with a newer network, puzzle
 * suites, opening checks, a move for a mid-game position at full search strength.
 *
 * Position i = (board[i], sign_to_move[i], serial[i], default 0) is searched exactly as a freshly created self-play GameGenerator would
 * search for its first move after an opening that produced this board: empty tree, empty solver table, the solver's generation counting
 * from 0 (the first search makes it 1), nn_queued 0, serial[i] as the noise / symmetry serial, move number = stones on the board, under the
 * AgxEngineConfig of agx_position_searcher_create.  The search ends when the engine's own move rule fires (root proven, or more root visits
 * than get_simulations_for_move allows); the result is the root at that moment — what the game's first AgxMoveRecord and root-edge snapshot
 * would hold.  Nothing is played.  The result is a function of the position, its serial and the configuration alone: not of the batch, of
 * the position's place in it, of the number of slots, of the slot that took it or of what that slot searched before.  One exception: the
 * arena reserve is shared by the pool, so whether a tree that outgrows every arena ends with status 2 can depend on its neighbours.
 * A position that is already decided (five in a row on the board) is NOT detected (Tree::setBoard does not detect it either): it is
 * searched like any other.
 *
 * The pool has cfg.n_games slots.  A free slot takes the next position off a device-side cursor, a slot whose search has ended writes its
 * outputs and is free again in the same step; the host only launches steps.
 * ---------------------------------------------------------------------------------------------- */
typedef struct AgxPositionSearcher AgxPositionSearcher;

enum
{ /* status words */
	AGX_POSSEARCH_STATUS_BAD_INPUT = 1,    /* a cell value above 2 or a sign other than 1 / 2: zeroed outputs, no edge (edge_index -1), nothing was searched */
	AGX_POSSEARCH_STATUS_ENGINE_ERROR = 2, /* the slot's engine error word was set (info[3]; e.g. the arena reserve ran out): zeroed outputs but info */
	AGX_POSSEARCH_STATUS_STEP_LIMIT = 3    /* max_steps steps without the move rule firing: the root as it stands (leaves in flight dropped, their
	                                          virtual losses taken back), or zeros with n_edges 0 when there is no root yet */
};

typedef struct AgxPositionSearchOutputs
{ /* device addresses; any of them may be NULL.  `cells` = board_size^2; rows are always written whole */
	int32_t* status;      /* [n] 0 searched, or AGX_POSSEARCH_STATUS_* */
	int32_t* root;        /* [n][4] root visits, root Score raw bits, root flags as AgxMoveRecord.root_flags, number of root edges */
	float* root_value;    /* [n][2] (win, draw) of the root node */
	uint16_t* best_move;  /* [n] the pick of cfg.final_selector (Move::toShort; the engine's own code path and tie rule), 0 without edges */
	int32_t* visits;      /* [n][cells] per cell: the root edge on that cell; 0 / 0.0f where the root has no edge */
	float* prior;         /* [n][cells] */
	float* q;             /* [n][cells][2] (win, draw) */
	uint16_t* score;      /* [n][cells] Score raw bits */
	int16_t* edge_index;  /* [n][cells] the cell's place in the root's edge order, -1 where the root has no edge */
	uint16_t* pv;         /* [n][max_pv] the walk of agx_engine_principal_variation from the root, zeros behind it */
	int32_t* pv_length;   /* [n] */
	int32_t* info;        /* [n][4] nodes in the tree, edges in the tree, steps the slot spent on the position, engine error code */
} AgxPositionSearchOutputs;

/* cfg->n_games is the number of slots.  AGX_ERR_UNSUPPORTED: match_mode, search_threads > 1, search_buffers > 1; everything else as
 * agx_engine_create refuses it.  The searcher owns an AgxEngine (its record pools are kept at their minimum: nothing is recorded). */
int agx_position_searcher_create(const AgxEngineConfig* cfg, AgxPositionSearcher** out);
int agx_position_searcher_destroy(AgxPositionSearcher* ps);
/* slots and everything the searcher allocated on the device; either output may be NULL */
int agx_position_searcher_info(const AgxPositionSearcher* ps, int* slots, uint64_t* device_bytes);
/* The owned engine, for agx_engine_stats, agx_engine_set_max_simulations and agx_engine_set_batch_size ONLY (and the read-only queries
 * agx_engine_game_info / agx_engine_principal_variation of a slot between two stages): stepping it, agx_engine_begin or agx_engine_set_board
 * on it break the searcher. */
int agx_position_searcher_engine(AgxPositionSearcher* ps, AgxEngine** out);
/* Records the job — d_boards uint8[n][cells] (0 empty, 1 cross, 2 circle), d_signs uint8[n] (1 cross / 2 circle to move), d_serials
 * int32[n] or NULL (all 0), the outputs, max_pv plies of principal variation per position — and loads the first positions into the slots.
 * Launches on `stream`, nothing synchronised; the arrays must stay valid until the job has finished.  n == 0 is a valid no-op (nothing is
 * launched, nothing written).  max_steps <= 0 selects the default
 *     (max_simulations + 2) * (2 * max_batch_size + 1) + 6
 * steps per position: a search adds a root visit in every step that expands a batch, the move rule fires after at most
 * max_simulations + 2 of them, a batch reaches its expand stage after at most max_batch_size solver launches that yield (each solves at
 * least one leaf) plus max_batch_size launches that park a solve (each solve is parked at most once) plus its own, and a tree changes its
 * arena class at most 5 times at one step each (and one step to spare).  AGX_ERR_INVALID: a null searcher or `out`, n or max_pv negative, null boards or signs
 * with n > 0; AGX_ERR_STATE: the previous job has not finished. */
int agx_position_searcher_begin(AgxPositionSearcher* ps, int n, const uint8_t* d_boards, const uint8_t* d_signs, const int32_t* d_serials,
		const AgxPositionSearchOutputs* out, int max_pv, int max_steps, void* stream);
/* One step in stages, for callers with an evaluator of their own: select_solve (agx_engine_select_solve), then the positions listed in
 * agx_position_searcher_buffers (the engine's AgxEngineBuffers) are evaluated — by the caller, or by _evaluate with a network —, then
 * expand (agx_engine_expand_group without its arena service), then harvest: the slots whose search has ended write their outputs, grown
 * arenas are serviced and free slots take the next positions.  All launches on `stream`, nothing synchronised. */
int agx_position_searcher_select_solve(AgxPositionSearcher* ps, void* stream);
int agx_position_searcher_buffers(AgxPositionSearcher* ps, AgxEngineBuffers* out);
int agx_position_searcher_evaluate(AgxPositionSearcher* ps, AgxNet* net, void* stream);
int agx_position_searcher_expand(AgxPositionSearcher* ps, void* stream);
int agx_position_searcher_harvest(AgxPositionSearcher* ps, void* stream);
/* the position every slot works on, -1 for a free slot: int[slots]; waits for `stream` only */
int agx_position_searcher_slots(AgxPositionSearcher* ps, void* stream, int* h_position_of_slot);
/* positions of the job whose outputs are written; waits for `stream` only */
int agx_position_searcher_finished(AgxPositionSearcher* ps, void* stream, int* count);
/* begin, then whole steps with `net` until all n positions are finished.  The finished counter is read behind the stream every few steps
 * (the host sleeps between polls as agx_event_synchronize does, a few steps stay queued meanwhile); no device-wide synchronisation; the
 * stream is drained on return.  The loop ends: every position finishes or reaches its step limit. */
int agx_position_searcher_search(AgxPositionSearcher* ps, AgxNet* net, int n, const uint8_t* d_boards, const uint8_t* d_signs,
		const int32_t* d_serials, const AgxPositionSearchOutputs* out, int max_pv, int max_steps, void* stream);
/* Calls on one searcher share its pool: a call on another stream than the previous one is ordered behind it on the device. */

/* Format-201 samples out of the searcher: the harvest stage quantises the root of position i to the reference's SearchDataStorage_v201
 * bytes (csrc/sample_v201.hpp) at d_bytes + i * stride — exactly what the first move record of a self-play game that started from the
 * position would carry: the three scales from the maxima over the root's edges, the root's score, move number = stones on the board, the
 * root's flags, the entry count, then 6 bytes per kept cell in cell order (an edge with visits or a proven score; and any cell 255 or more
 * cells past the previous entry) — and the byte count into d_sizes[i].  Status 0 and status 3 with a root write the sample of the root as
 * it stands; status 1, 2 and 3 without a root write size 0 and leave the bytes alone.  stride >= 16 + 6 * cells, a multiple of 4
 * (AGX_ERR_INVALID otherwise); a NULL sink, or one with either pointer NULL, means no samples: the calls are then the ones above. */
typedef struct AgxPositionSampleSink
{ /* device addresses */
	uint8_t* d_bytes;  /* [n][stride] */
	int stride;
	int32_t* d_sizes;  /* [n] */
} AgxPositionSampleSink;
int agx_position_searcher_begin_ex(AgxPositionSearcher* ps, int n, const uint8_t* d_boards, const uint8_t* d_signs, const int32_t* d_serials,
		const AgxPositionSearchOutputs* out, const AgxPositionSampleSink* sink, int max_pv, int max_steps, void* stream);
int agx_position_searcher_search_ex(AgxPositionSearcher* ps, AgxNet* net, int n, const uint8_t* d_boards, const uint8_t* d_signs,
		const int32_t* d_serials, const AgxPositionSearchOutputs* out, const AgxPositionSampleSink* sink, int max_pv, int max_steps, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Saved games reanalysed on the device: the positions of a fragment's samples searched again with the current network, a buffer of the
 * same games with fresh policy / action-value / score targets (csrc/training_batch.hip: k_dataset_positions; the sink above;
 * csrc/game_buffer.cpp).  Moves and outcome stay the game's.
 * ---------------------------------------------------------------------------------------------- */
/* The positions of n samples (fragment, game, sample; the augmentation is ignored) as the searcher takes them: d_boards uint8[n][cells]
 * (0 / 1 / 2, row-major: the game's first move_number moves), d_signs uint8[n] (the colour of move move_number).  One launch on `stream`,
 * one wavefront per sample, on the fragment bytes resident on the device; indices are validated first, as by agx_dataset_load_batch. */
int agx_dataset_positions(AgxDataset* dataset, int n, const AgxDatasetSample* h_samples, uint8_t* d_boards, uint8_t* d_signs, void* stream);
/* Appends the format-201 game h_game[size] to `out` with sample k replaced by h_samples[k][0 .. h_sizes[k]) where h_sizes[k] > 0 (the old
 * bytes stay where it is 0); move list, outcome, rows and cols are kept.  Host code only.  AGX_ERR_INVALID: a truncated game, n_samples
 * other than the game's count, a replacement that is no whole sample or whose move number differs from the old sample's, a game of another
 * board than the buffer's. */
int agx_game_buffer_add_reanalysed(AgxGameBuffer* out, const uint8_t* h_game, size_t size, int n_samples, const uint8_t* const* h_samples,
		const int32_t* h_sizes);

typedef struct AgxReanalyseOptions
{
	int chunk;        /* positions per searcher job; 0 = 16384 */
	int serial_base;  /* position j of the pass (samples in (game, sample) order) is searched with serial serial_base + j */
	int max_steps;    /* as agx_position_searcher_begin; <= 0: its default */
} AgxReanalyseOptions;
typedef struct AgxReanalyseStats
{
	int64_t games, samples;
	int64_t replaced;     /* samples with status 0: their bytes are the fresh search's */
	int64_t kept;         /* every other sample: the old bytes (a truncated search is no training target) */
	int64_t status[4];    /* samples per AGX_POSSEARCH_STATUS_* (0 = searched) */
	int64_t steps;        /* sum over the samples of the steps their slot spent on them */
} AgxReanalyseStats;
/* The whole pass over one fragment: `chunk` positions at a time agx_dataset_positions, agx_position_searcher_search_ex with a sink, one
 * copy of sizes, status words, step counts and the used sample bytes into pinned memory; a game is handed to
 * agx_game_buffer_add_reanalysed once all its samples are in.  The result does not depend on `chunk` or on the searcher's slot count.
 * `options` NULL: all defaults; `stats` may be NULL.  AGX_ERR_INVALID before anything is launched: a null argument, a fragment that is
 * not loaded, rules or board size of dataset, searcher and `out` that differ.  The call waits for `stream`. */
int agx_dataset_reanalyse(AgxDataset* dataset, int fragment, AgxPositionSearcher* searcher, AgxNet* net, AgxGameBuffer* out,
		const AgxReanalyseOptions* options, AgxReanalyseStats* stats, void* stream);

/* Raw device-memory helpers so that non-HIP hosts (ctypes, cgo) can stage buffers. */
int agx_malloc(void** d_ptr, size_t bytes);
int agx_free(void* d_ptr);
int agx_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes);
int agx_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes);
int agx_memset(void* d_ptr, int value, size_t bytes);
int agx_device_synchronize(void);

/* Timing of work enqueued on `stream` with HIP events recorded on that same stream. */
typedef struct AgxTimer AgxTimer;
int agx_timer_create(AgxTimer** out);
int agx_timer_start(AgxTimer* t, void* stream);
int agx_timer_stop(AgxTimer* t, void* stream);
int agx_timer_elapsed_ms(AgxTimer* t, float* ms); /* synchronises on the stop event */
/* the same without waiting: *ready = 0 (and *ms untouched) while the timed work has not finished.  What NNEvaluator::asyncEvaluateGraphLaunch's
 * end-time estimate reads (NNEvaluator.cpp:197-206): a launch loop must not block on its previous network launch for a statistic. */
int agx_timer_poll_ms(AgxTimer* t, float* ms, int* ready);
int agx_timer_destroy(AgxTimer* t);

#ifdef __cplusplus
}
#endif
#endif /* AGX_H_ */
