/*
 * engine.hip — the device-resident self-play engine: its kernels and, at the end, the launch layer over them (engine_launch.hpp).  The host
 * objects and the C ABI (include/agx.h) are in engine_host.cpp, position_solver.cpp and position_searcher.cpp.
 *
 * One step of the pool = what GameGenerator::generate does for every game of a GeneratorThread
 * (src/selfplay/GameGenerator.cpp:79-118, src/selfplay/GeneratorManager.cpp:124-141), as four launches:
 *
 *   k_solve<.., FUSED>   one wave per game, two stages back to back (a game's stages depend on no other game):
 *              Search::select          (Search.cpp:117-158)   up to `batch` PUCT descents per game, virtual loss
 *              Search::solve           (Search.cpp:159-183)   threat solver on every new leaf + NN feature encode,
 *              Search::scheduleToNN    (Search.cpp:184-199)   compacts the positions that need the network
 *              (k_select + k_solve<.., false> are the same stages as two launches: agx_engine_select_group / _solve_group, tournament pools)
 *   (network)  NNEvaluator::evaluate                         agx_nn_forward over the compacted list (nn_forward.hip)
 *   k_expand   Search::generateEdges / expand / backup (Search.cpp:206-232) and the move rule (GameGenerator.cpp:97-103)
 *   k_advance  GameGenerator::make_move + prepare_search (:145-185): final selector, sample record, outcome test (incl. renju
 *              fouls), NodeCache::cleanup as a keep-test + prefix-sum compaction into the game's other arena
 *   k_assign_openings / k_restart   finished games take the next openings in game order (GAME_NOT_STARTED -> next game)
 *   k_arena_service / _copy   trees that outgrew their arenas move into larger ones (NodeCache::resize, ObjectPool growth)
 *
 * Everything stays in HBM between steps; the host only enqueues launches.  One wavefront per game for the sequential
 * tree work (the games of different slots share nothing, the batch inside a game is order-dependent through virtual loss); k_advance
 * uses a 1024-thread workgroup per game because compaction is data parallel.  A slot's games follow one another on one generator:
 * its task slots and its solver's generation go on from game to game (begin_game), as a GameGenerator's do.
 */
#include "agx_internal.hpp"
#include "engine_types.hpp"
#include "engine_launch.hpp"
#include "dev_mcts.hpp"
#include "renju_static.hpp"
#include "root_noise.hpp"
#include "sample_v201.hpp"

#include <cstring>
#include <algorithm>

using namespace agx;
using namespace agx::dev;

namespace
{
	/* ------------------------------------------------------------------------------------------------------------ */
	/* Search::select for one task buffer: `g` owns the buffer (its GameState `ls` carries the batch bookkeeping and statistics), `tg` owns
	 * the tree (its GameState `gs`).  Self-play: tg == g.  Tournament search (shared_tree): every search thread g descends tree 0. */
	__device__ __forceinline__ void select_batch(EngineDev &E, int tg, int g, int lane, uint8_t *sh_board, u64 *sh_cboard, const u64 *sh_keys)
	{
		GameState &gs = E.games[tg];
		GameState &ls = E.games[g];
		DNode *nodes = nodes_of(E, tg, gs.arena);
		DEdge *edges = edges_of(E, tg, gs.arena);
		const int *ht = ht_of(E, tg);
		const int n = E.n;

		int n_tasks = ls.n_tasks;
		int trials = 2 * E.batch_limit; // Search.cpp:119: twice the buffer's current size (Search::setBatchSize)
		unsigned long long st_levels = 0, st_edges = 0, st_leaks = 0, st_proven = 0, st_dup = 0;
		while (n_tasks < E.batch_limit)
		{
			const int root = gs.root;
			const int sims = (root < 0) ? 0 : nodes[root].visits;
			if (sims > E.max_sims)
				break;
			if (E.noise_type != 0 && root >= 0 && !gs.noise_ready && nodes[root].n_edges > 0)
			{ // PUCTSelector::select's lazy noise initialisation on the first visit of an expanded root (EdgeSelector.cpp:1127-1137)
				if (lane == 0)
				{
					const DNode rn = nodes[root];
					const DEdge *root_edges = edges + rn.edge_begin;
					make_root_noise(E.noise_type, E.noise_weight, E.noise_seed, gs.opening_id, gs.n_moves, rn.n_edges, [&](int i) { return root_edges[i].prior; },
							E.noise + static_cast<size_t>(tg) * E.hw);
					gs.noise_ready = 1;
				}
				__threadfence_block();
				__syncthreads();
			}
			DTask &t = E.tasks[static_cast<size_t>(g) * E.batch + n_tasks];
			n_tasks++;
			// SearchTask::set (SearchTask.cpp:32-50)
			for (int i = lane; i < E.hw; i += 64)
				sh_board[i] = gs.board[i];
			if (lane < BWORDS)
				sh_cboard[lane] = gs.cboard[lane];
			__syncthreads();
			int path_len = 0, final_node = -1, out = 0, sign = gs.sign_to_move;
			u64 hash = gs.root_hash;
			int last_edge = -1;
			int node = root;
			// One dependent chain per level: edges of the node -> the chosen edge -> table slot -> the child's record.  The node
			// record is read ONCE (by the seek that found it), the chosen edge once, and the hash keys come from LDS.
			DNode nd;
			if (node >= 0)
				node_head(nd, nodes[node]);
			while (node >= 0)
			{
				if (path_len >= PATH_CAP)
				{
					if (lane == 0)
						ls.error = ERR_PATH_CAPACITY;
					break;
				}
				const int e = select_edge(E, nd, edges, lane, st_edges, (node == root && gs.noise_ready) ? E.noise + static_cast<size_t>(tg) * E.hw : nullptr);
				st_levels++;
				const DEdge ee = edges[e]; // as it was before this visit's virtual loss (what the leak test compares, Tree.cpp:75-85)
				const uint32_t mv = ee.move;
				const int s = mv & 3, cell = ((mv >> 2) & 127) * n + ((mv >> 9) & 127);
				const uint16_t flag_vl = static_cast<uint16_t>((ee.flag_vl & 0x8000u) | (((ee.flag_vl & 0x7FFF) + 1) & 0x7FFF));
				if (lane == 0)
				{ // SearchTask::append (SearchTask.cpp:52-60) + virtual loss (Tree.cpp:235-236)
					sh_board[cell] = static_cast<uint8_t>(s);
					sh_cboard[cell >> 5] |= static_cast<u64>(s) << (2 * (cell & 31));
					t.path_node[path_len] = node;
					t.path_edge[path_len] = e;
					nodes[node].vl = static_cast<int16_t>(nd.vl + 1);
					edges[e].flag_vl = flag_vl;
				}
				hash ^= sh_keys[3 + 3 * cell] ^ sh_keys[3 + 3 * cell + s] ^ sh_keys[sign] ^ sh_keys[3 - s];
				sign = 3 - s;
				path_len++;
				last_edge = e;
				__syncthreads();
				if (s_proven(ee.score))
				{
					out = 2;
					break;
				}
				DNode child;
				node = cache_seek_head(E, nodes, ht, hash, sh_cboard, sign, lane, child);
				final_node = node;
				if (node < 0 && lane == 0)
					edges[e].flag_vl = static_cast<uint16_t>(flag_vl | 0x8000u);
				if (has_leak(E, ee, node >= 0, child.score, child.win, child.draw))
				{
					out = 1;
					break;
				}
				nd = child;
			}
			// publish the task
			for (int i = lane; i < E.hw; i += 64)
				t.board[i] = sh_board[i];
			if (lane < BWORDS)
				t.cboard[lane] = sh_cboard[lane];
			if (lane == 0)
			{
				t.path_len = path_len;
				t.final_node = final_node;
				t.n_edges = 0;
				t.flags = t.flags & (TF_STATICALLY_SOLVED | TF_RECURSIVELY_SOLVED); // these two survive SearchTask::set
				t.sign_to_move = sign;
				t.score = s_unknown(0);
				t.win = 0.0f;
				t.draw = 0.0f;
				// (t.moves_left stays: SearchTask::set (SearchTask.cpp:32-50) resets the value, not the moves-left estimate — a proven-edge leaf, which neither
				//  the solver nor the network touches, backs up what the previous occupant of this task slot left behind, Tree.cpp:304)
				t.needs_nn = 0;
				t.hash = hash;
				if (out == 0 && path_len > gs.max_depth)
					gs.max_depth = path_len; // Tree.cpp:249 (REACHED_LEAF only)
			}
			__syncthreads();
			if (path_len == 0)
				break; // the root itself has to be evaluated
			for (int i = 0; i < n_tasks - 1; i++)
			{ // Search::is_duplicate (statistics only)
				const DTask &o = E.tasks[static_cast<size_t>(g) * E.batch + i];
				if (o.path_len > 0 && o.path_edge[o.path_len - 1] == last_edge)
				{
					st_dup++;
					break;
				}
			}
			if (out == 1)
			{
				correct_information_leak(nodes, edges, t, path_len, final_node, lane);
				cancel_virtual_loss(nodes, edges, t, path_len, lane);
				st_leaks++;
				n_tasks--;
			}
			if (out == 2 && lane == 0)
			{ // Search.cpp:139-150
				const uint32_t sc = edges[last_edge].score;
				float w, d;
				s_to_value(sc, w, d);
				t.final_node = -1;
				t.sign_to_move = 3 - sign;
				t.score = sc;
				t.win = w;
				t.draw = d;
				t.flags |= TF_BY_SOLVER | TF_SKIP_EDGE_GENERATION;
			}
			if (out == 2)
				st_proven++;
			__syncthreads();
			if (--trials <= 0)
				break;
		}
		if (lane == 0)
		{
			ls.n_tasks = n_tasks;
			ls.stats[2] += st_leaks;
			ls.stats[3] += st_proven;
			ls.stats[6] += st_levels;
			ls.stats[7] += st_edges;
			ls.stats[9] += st_dup;
		}
	}
	__global__ __launch_bounds__(64) void k_select(EngineDev E)
	{
		__shared__ uint8_t sh_board[MAXHW];
		__shared__ u64 sh_cboard[BWORDS];
		__shared__ u64 sh_keys[3 * (1 + MAXHW)]; // FullZobristHashing keys of the node cache: four per level, from LDS instead of L2
		const int g = E.g0 + blockIdx.x, lane = threadIdx.x;
		const int tg = E.shared_tree ? 0 : g;
		GameState &gs = E.games[tg];
		if (!gs.active || gs.error != 0 || gs.outcome != 0 || gs.grow_pending)
			return; // (grow_pending: the previous batch still waits for its expansion in larger arenas)
		use_game_arenas(E, tg);
		if (E.match_merged)
			use_player_search(E, g);
		for (int i = lane; i < 3 * (1 + E.hw); i += 64)
			sh_keys[i] = E.nc_keys[i];
		if (!E.shared_tree)
		{
			if (!gs.solve_pending)
				select_batch(E, g, g, lane, sh_board, sh_cboard, sh_keys);
			return;
		}
		// tournament search: the search threads take the tree one after the other (SearchThread.cpp:124-129), in thread order
		// (double-buffered search: this launch's buffer of every thread — the other buffer's leaves keep their virtual losses meanwhile)
		for (int t = E.grp_first; t < E.grp_first + E.grp_count; t++)
		{
			if (E.games[t].error == 0)
				select_batch(E, 0, t, lane, sh_board, sh_cboard, sh_keys);
			__syncthreads();
		}
	}

	/* ------------------------------------------------------------------------------------------------------------ */
	/* Where a solve keeps what does not fit into LDS: `area` indexes the per-game spill areas (the game itself, or for speculative solves —
	 * several tasks of one game at once — the wave's own area behind the games'); `overlay` != nullptr makes the solve speculative
	 * (dev_solver.hpp: the table is only read, every touched bucket lives in the overlay). */
	/*
	 * Parking (round 5).  A launch of k_search_spec ends when its last solve does, and a few solves per launch run several times the
	 * average (renju: positions whose move generation tests dozens of cells for fouls — 0.5 % of the leaves take 5-9 ms against 1.7 on average,
	 * profiles/r05_c5_search_launch_timeline.txt): the compute units of the slice idle for half the launch behind a handful of waves.  Once
	 * SPEC_PARK_FRACTION of the launch's games are done and the queue has run dry, a speculative solve that is still running is PARKED at its
	 * next command boundary: the solver's LDS state (everything the frame machine needs: it already yields to the caller for every stone) goes
	 * into a park buffer, the in-use parts of the wave's HBM tails (undo snapshots, action stack / frame / list tails) into the buffer's own
	 * spill area, the game sits this step out like a game whose commit was deferred (solve_pending), and the next launch — which queues the
	 * game's unsolved leaves as it does for a deferred game — finds the task's park buffer and takes the solve up where it stopped, in any
	 * wave.  The solve's result cannot depend on it: the machine continues from the same state against the same table (the game's table is not
	 * written while its batch is in flight).  A solve is parked at most once (it then has a whole launch in front of it), and only when a
	 * buffer is free.  Pacing only, like the yield rule.
	 */
	struct ParkCtl
	{
			int count;     // games of the launch
			int threshold; // games done from which running solves are parked (0x7FFFFFFF: never)
	};
	/* what a solve keeps in spill area `from`, copied to area `to`: the parts in use (or a superset of them) */
	template<class SH>
	__device__ __forceinline__ void park_copy_tails(const SH &sh, const EngineDev &E, int from, int to, int lane)
	{
		lane = fresh_lane(lane); // (cold code: none of its per-lane addresses is to be computed at the top of the kernel and kept in registers or scratch)
		{ // undo snapshots: one 512-byte level per stone on the board
			const u64 *a = E.snap_spill + static_cast<size_t>(from) * (E.hw + 2) * 64;
			u64 *b = E.snap_spill + static_cast<size_t>(to) * (E.hw + 2) * 64;
			const int words = min(sh.depth, E.hw + 2) * 64;
			for (int i = lane; i < words; i += 64)
				b[i] = a[i];
		}
		{ // action stack beyond its LDS part
			const uint32_t *a = E.act + static_cast<size_t>(from) * E.act_cap;
			uint32_t *b = E.act + static_cast<size_t>(to) * E.act_cap;
			const int top = min(sh.stack_max, E.act_cap);
			for (int i = SH::ACT_LDS + lane; i < top; i += 64)
				b[i] = a[i];
		}
		{ // frames beyond the LDS-resident ones (32 bytes each)
			const u64 *a = reinterpret_cast<const u64*>(E.frame_spill) + static_cast<size_t>(from) * MAX_FRAMES * 4;
			u64 *b = reinterpret_cast<u64*>(E.frame_spill) + static_cast<size_t>(to) * MAX_FRAMES * 4;
			const int top = min(sh.level + 2, MAX_FRAMES) * 4;
			for (int i = SH::FRAMES * 4 + lane; i < top; i += 64)
				b[i] = a[i];
		}
		{ // threat-list entries beyond a list's LDS capacity
			const uint16_t *a = E.list_spill + static_cast<size_t>(from) * 20 * MAXHW;
			uint16_t *b = E.list_spill + static_cast<size_t>(to) * 20 * MAXHW;
			for (int st = 0; st < 20; st++)
			{
				const int side = st / 10, type = st % 10;
				if (type < 2)
					continue;
				const int cnt = sh.count[side][type];
				for (int i = SH::list_cap(type) + lane; i < cnt; i += 64)
					b[st * SH::HW + i] = a[st * SH::HW + i];
			}
		}
	}
	template<class SH>
	__device__ __forceinline__ void park_point_tails_at(SH &sh, const EngineDev &E, int area)
	{ // HBM tails of the LDS-resident threat lists and frames (dev_solver.hpp: list_get / frame_get), undo snapshots (lane 0)
		sh.spill_lists = E.list_spill + static_cast<size_t>(area) * 20 * MAXHW; // (stride of list_get / list_set: SolverSharedT::HW <= MAXHW whatever the kernel instantiation)
		sh.spill_frames = reinterpret_cast<Frame*>(E.frame_spill) + static_cast<size_t>(area) * MAX_FRAMES;
		sh.snap = E.snap_spill + static_cast<size_t>(area) * (E.hw + 2) * 64; // undo snapshots, one level per stone on the board (dev_solver.hpp)
	}
	/* every lane: is it time to park (wave-uniform result)?  One counter read while the launch is busy, three more once the threshold is reached. */
	__device__ __forceinline__ bool park_wanted(const EngineDev &E, const ParkCtl &p, int lane)
	{
		const int *c_done = E.counters + E.yield_counter;                 // games of the launch that are done with their batch
		const int *c_queue = E.counters + SPEC_COUNTER0 + 4 * E.spec_group; // [0] select cursor, [1] queue head, [2] queue tail, [3] games selected
		int yes = 0;
		if (lane == 0 && __hip_atomic_load(c_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= p.threshold)
			yes = (__hip_atomic_load(c_queue + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= p.count
					&& __hip_atomic_load(c_queue + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= __hip_atomic_load(c_queue + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ? 1 : 0;
		return __builtin_amdgcn_readfirstlane(yes) != 0;
	}
	/* claims a free park buffer for task `slot` (every lane gets the same answer: the buffer's index, or -1) */
	__device__ __forceinline__ int park_claim(const EngineDev &E, int slot, int lane)
	{
		int b = -1;
		if (lane == 0)
			for (int probe = 0; probe < 8 && b < 0; probe++)
			{
				const int i = (slot * 7 + probe * 13) & (SPEC_PARK_POOL - 1);
				if (atomicCAS(&E.park_owner[i], 0, slot + 1) == 0)
					b = i;
			}
		return __builtin_amdgcn_readfirstlane(b);
	}
	/* forgets what game g has parked (the game is restarted, its board set from outside, its pending batch cancelled): lane 0 / one thread.
	 * With a parked solve the game's OTHER leaves of that launch stay "solved speculatively" (SpecTask::solved, overlay uncommitted) across
	 * launches; whoever discards the batch discards those too, or a later batch's proven-edge task in the same slot — which the solver never
	 * sees — would be taken for one by spec_commit_game and have a stale overlay written into the table. */
	__device__ __forceinline__ void park_forget_game(const EngineDev &E, int g)
	{
		for (int k = 0; k < E.batch; k++)
		{
			const int b = E.park_slot[g * E.batch + k];
			if (b != 0)
			{
				E.park_slot[g * E.batch + k] = 0;
				__hip_atomic_store(&E.park_owner[b - 1], 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
			}
			if (E.spec_on)
				E.spec_tasks[g * E.batch + k].solved = 0;
		}
	}
	/* A serial solve launch (k_solve: Search::solve with a time limit, or solve() behind flush_select()) on a pool whose last speculative launch
	 * left game g waiting (a deferred commit or a parked solve): the leaves of the batch that were solved speculatively but never committed go
	 * back to what the select stage made of them — as spec_commit_game's defer path does — and the parked solve is dropped, so that the serial
	 * loop solves every pending leaf on the table itself, in batch order.  lane 0 / one thread. */
	__device__ __forceinline__ void spec_discard_pending(const EngineDev &E, int g)
	{
		if (!E.spec_on)
			return;
		for (int k = 0; k < E.batch; k++)
		{
			SpecTask &h = E.spec_tasks[g * E.batch + k];
			if (h.solved != 0)
			{
				DTask &t = E.tasks[static_cast<size_t>(g) * E.batch + k];
				t.flags = h.flags0;
				t.win = 0.0f;
				t.draw = 0.0f;
				t.moves_left = h.moves_left0;
			}
		}
		park_forget_game(E, g); // (also clears SpecTask::solved)
	}
	/* returns true when the solve was parked (nothing of `t` has been written then), false when it is finished */
	template<bool RENJU, class SH>
	__device__ __forceinline__ bool solve_task(SH &sh, const EngineDev &E, int g, DTask &t, int slot, int generation, int lane, unsigned long long &solver_nodes,
			int area, u64 *overlay = nullptr, const ParkCtl *park = nullptr)
	{ // AlphaBetaSearch::solve (AlphaBetaSearch.cpp:77-156)
		uint32_t *act = E.act + static_cast<size_t>(area) * E.act_cap;
		u64 *tt = E.tt + static_cast<size_t>(g % E.tt_mod) * (E.tt_bucket_mask + 1ull) * 8ull; // (double-buffered search: both buffers of a thread use its one solver)
		const int parked_in = (park != nullptr) ? __builtin_amdgcn_readfirstlane(E.park_slot[slot]) : 0; // park buffer + 1 this task's solve waits in
		int depth_first = 0, stack_before_first = 0;
		if (parked_in != 0)
		{ // ---- take a parked solve up again: LDS state and loop variables out of the buffer, the HBM tails into this wave's area ----
			static_assert(sizeof(SH) % 8 == 0 && sizeof(SH) / 8 <= SPEC_PARK_WORDS - 8, "park buffer holds the solver's LDS state");
			const u64 *src = E.park_lds + static_cast<size_t>(parked_in - 1) * SPEC_PARK_WORDS;
			u64 *lds = reinterpret_cast<u64*>(&sh);
			for (int i = fresh_lane(lane); i < static_cast<int>(sizeof(SH) / 8); i += 64)
				lds[i] = global_view(src)[i];
			depth_first = static_cast<int>(src[SPEC_PARK_WORDS - 8]);
			stack_before_first = static_cast<int>(src[SPEC_PARK_WORDS - 7]);
			wave_sync();
			park_copy_tails(sh, E, E.park_area0 + parked_in - 1, area, lane);
			if (lane == 0)
			{
				park_point_tails_at(sh, E, area);
				sh.pf_valid = 0; // (the bucket prefetched for the next frame was in registers)
				E.park_slot[slot] = 0;
			}
			__threadfence(); // the copies are done before the buffer can be claimed again
			wave_sync();
			if (lane == 0)
				__hip_atomic_store(&E.park_owner[parked_in - 1], 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
		}
		else
		{
		if (lane == 0)
		{
			park_point_tails_at(sh, E, area);
			sh.ov_on = (overlay != nullptr) ? 1 : 0;
			sh.ov_data = overlay;
			sh.ov_count = 0;
			sh.ov_overflow = 0;
			sh.pf_slot = -1;
		}
		if (lane < OV_CAP / 32)
			sh.ov_dirty[lane] = 0;
		}
#ifdef AGX_SOLVER_PROFILE
		unsigned long long c0 = wall_clock64(), c_run = 0, c_place = 0, n_place = 0;
		unsigned long long c1 = c0, t_forbidden = 0;
#endif
		if (parked_in == 0)
		{
		solver_set_board(sh, E, t.board, t.sign_to_move, lane);
		solver_encode_features(sh, E, E.nn_features + static_cast<size_t>(slot) * E.hw, lane);
		#ifdef AGX_SOLVER_PROFILE
		const unsigned long long c_enc = wall_clock64();
		#endif
		if (RENJU)
			solver_encode_forbidden(sh, E, E.nn_features + static_cast<size_t>(slot) * E.hw, lane);
		#ifdef AGX_SOLVER_PROFILE
		c1 = wall_clock64();
		t_forbidden = c1 - c_enc; // renju: the forbidden-move bits of the network input (probes place and remove stones)
		#endif
		u64 lo = 0, hi = 0;
		for (int i = lane; i < E.hw; i += 64)
		{
			const int v = sh.board[i];
			if (v == 1 || v == 2)
			{
				lo ^= zobrist_word(E.zobrist_seed, 2 * (2 * i + v - 1));
				hi ^= zobrist_word(E.zobrist_seed, 2 * (2 * i + v - 1) + 1);
			}
		}
		lo = wave_reduce_xor64(lo);
		hi = wave_reduce_xor64(hi);
		if (lane == 0)
		{
			sh.hash_lo = lo;
			sh.hash_hi = hi;
			sh.node_counter = 0;
			sh.stack_offset = 0;
			sh.stack_max = 0;
			sh.error = 0;
			sh.pf_valid = 0;
#ifdef AGX_SOLVER_PROFILE
			for (int i = 0; i < 8; i++)
				sh.prof[i] = 0;
			for (int i = 0; i < 24; i++)
				sh.dprof[i] = 0;
#endif
			Frame &f = sh.frames[0];
			f.base = 0;
			f.size = 0;
			f.baseline = static_cast<uint16_t>(s_unknown(0));
			f.must_defend = f.has_initiative = f.fully_expanded = 0;
		}
		wave_sync();
		}
		uint32_t result = s_unknown(0);
		u64 pf_word = 0; // lanes 0-7: the transposition-table bucket prefetched for the frame about to be entered
		uint8_t pf_pattern = 0; // pattern-table entries prefetched for the stone about to be placed / removed (dev_solver.hpp:pattern_prefetch)
		int pf_pattern_tag = -1; // move | add << 16 they belong to
		u64 pf_snap = 0; // an undo's snapshot word, requested by the frame machine when the node returns (tag: the move, add bit clear)
		// a solve may be parked once, and not in a launch in which nothing can be gained by it
		const bool may_park = (park != nullptr) && (parked_in == 0) && (park->threshold != 0x7FFFFFFF) && (overlay != nullptr);
		int turns = 0;
		for (int depth = depth_first; depth <= E.tss_max_depth; depth += 4)
		{
			int stack_before = 0;
			if (parked_in != 0 && depth == depth_first)
				stack_before = stack_before_first; // (the iteration the solve was parked in goes on)
			else if (lane == 0)
			{
				stack_before = sh.stack_max;
				Frame &f = sh.frames[0];
				f.depth_remaining = depth;
				f.alpha = 0x0000u;
				f.beta = 0xFFFFu;
				f.i = 0;
				sh.level = 0;
				sh.phase = 0;
				sh.pending_value = 0;
			}
			wave_sync();
			while (true)
			{
				if (may_park && ((++turns) & 15) == 0 && park_wanted(E, *park, lane))
				{ // ---- park: between two commands everything the machine needs is in LDS ----
					const int b = park_claim(E, slot, lane);
					if (b >= 0)
					{
						u64 *dst = E.park_lds + static_cast<size_t>(b) * SPEC_PARK_WORDS;
						const u64 *lds = reinterpret_cast<const u64*>(&sh);
						for (int i = fresh_lane(lane); i < static_cast<int>(sizeof(SH) / 8); i += 64)
							global_view(dst)[i] = lds[i];
						const int sb = __builtin_amdgcn_readfirstlane(stack_before); // (lane 0's)
						if (lane == 0)
						{
							dst[SPEC_PARK_WORDS - 8] = static_cast<u64>(depth);
							dst[SPEC_PARK_WORDS - 7] = static_cast<u64>(sb);
						}
						park_copy_tails(sh, E, area, E.park_area0 + b, lane);
						__threadfence();
						if (lane == 0)
						{
							GameState &pg = E.games[g];
							E.park_slot[slot] = b + 1;
							pg.solve_pending = 1; // (solve_pos stays: 0, or where a deferred game's batch went on)
							atomicAdd(&pg.spec_stats[3], 1ull);
						}
						__threadfence();
						wave_sync();
						return true;
					}
				}
#ifdef AGX_SOLVER_PROFILE
				const unsigned long long r0 = wall_clock64();
#endif
				pf_pattern_tag = -1;
				const int cmd_now = solver_run<RENJU>(sh, E, act, tt, generation, lane, pf_word, pf_pattern, pf_pattern_tag, pf_snap);
				if (lane == 0)
					sh.cmd = cmd_now;
				wave_sync();
#ifdef AGX_SOLVER_PROFILE
				const unsigned long long r1 = wall_clock64();
				c_run += r1 - r0;
#endif
				const int cmd = sh.cmd;
				if (cmd == CMD_ADD)
					solver_place(sh, E, static_cast<uint32_t>(sh.cmd_move), true, lane, pf_pattern_tag == (sh.cmd_move | 0x10000), pf_pattern);
				else if (cmd == CMD_UNDO)
					solver_place(sh, E, static_cast<uint32_t>(sh.cmd_move), false, lane, pf_pattern_tag == sh.cmd_move, pf_pattern, pf_pattern_tag == sh.cmd_move, pf_snap);
				else
					break;
#ifdef AGX_SOLVER_PROFILE
				c_place += wall_clock64() - r1;
				n_place++;
#endif
			}
			int stop = 0;
			if (lane == 0)
			{
				const uint32_t r = static_cast<uint32_t>(sh.result_score);
				stop = (sh.frames[0].size == 0 || s_proven(r) || sh.node_counter >= E.tss_max_nodes || sh.stack_max == stack_before || sh.error != 0) ? 1 : 0;
				if (E.solve_time_ticks != 0ull && wall_clock64() >= sh.time_deadline)
					stop = 1; // AlphaBetaSearch.cpp:111
			}
			stop = __builtin_amdgcn_readfirstlane(stop);
			result = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(sh.result_score));
			wave_sync();
			if (stop)
				break;
		}
		const int size = sh.frames[0].size;
		for (int i = lane; i < size; i += 64)
		{
			const uint32_t a = act_get(sh, act, i);
			t.emove[i] = static_cast<uint16_t>(a & 0xFFFFu);
			t.escore[i] = static_cast<uint16_t>(a >> 16);
		}
		if (lane == 0)
		{
			t.n_edges = size;
			t.score = result;
			if (s_proven(result))
			{
				float w, d;
				s_to_value(result, w, d);
				t.win = w;
				t.draw = d;
				t.moves_left = static_cast<float>(s_distance(result));
				t.flags |= TF_RECURSIVELY_SOLVED;
			}
			if (sh.frames[0].must_defend)
				t.flags |= TF_MUST_DEFEND;
			if ((sh.node_counter & NODE_COUNT_MASK) <= 1)
				t.flags |= TF_STATICALLY_SOLVED;
			t.flags |= TF_BY_SOLVER;
			if (sh.error != 0 && sh.error != ERR_OVERLAY)
				E.games[g].error = sh.error;
		}
		solver_nodes += static_cast<unsigned long long>(sh.node_counter & NODE_COUNT_MASK);
#ifdef AGX_SOLVER_PROFILE
		if (lane == 0)
		{
			GameState &pg = E.games[g];
			pg.prof[0] += c1 - c0;               // set_board + encode
			pg.prof[1] += c_run;                 // lane-0 frame machine (move generation, table probes, ordering)
			pg.prof[2] += c_place;               // place / remove stone
			pg.prof[3] += n_place;
			pg.prof[4] += wall_clock64() - c0;   // whole solve
			pg.prof[5] += 1;
			pg.prof[6] += sh.prof[0] | (sh.prof[1] << 32);
			pg.prof[7] += sh.prof[2] | (sh.prof[3] << 32);
			for (int i = 0; i < 24; i++)
				pg.dprof[i] += sh.dprof[i];
			pg.dprof[23] += t_forbidden;
		}
#endif
		wave_sync();
		return false;
	}

	/* Search::scheduleToNN (Search.cpp:184-199) for one game whose whole batch has been solved: input symmetries, the device-side queue of
	 * positions for the network.  Returns the number of positions scheduled. */
	template<class SH>
	__device__ __forceinline__ unsigned long long schedule_to_nn(SH &sh, const EngineDev &E, int g, GameState &gs, int n_tasks, int lane)
	{
		unsigned long long scheduled = 0;
		int queued = gs.nn_queued;
		for (int j = 0; j < n_tasks; j++)
		{
			DTask &t = E.tasks[static_cast<size_t>(g) * E.batch + j];
			const bool needs = (t.path_len == 0) || !s_proven(t.score);
			int symmetry = 0;
			if (needs && E.use_symmetries)
			{ // NNEvaluator::addToQueue + pack_to_network (NNEvaluator.cpp:134-141,244-262): augment the features in place
				symmetry = static_cast<int>(symmetry_mix(E.symmetry_seed ^ (static_cast<u64>(static_cast<uint32_t>(gs.opening_id)) << 32) ^ static_cast<uint32_t>(queued)) >> 61);
				if (symmetry != 0)
				{
					uint32_t *feat = E.nn_features + static_cast<size_t>(g * E.batch + j) * E.hw;
					__threadfence_block();
					for (int i = lane; i < E.hw; i += 64)
						sh.act[i] = feat[i]; // the action stack is idle between solves
					wave_sync();
					for (int i = lane; i < E.hw; i += 64)
					{
						int sr, sc;
						symmetry_source(symmetry, E.n, i / E.n, i % E.n, sr, sc);
						feat[i] = shuffle_feature_directions(sh.act[sr * E.n + sc], symmetry);
					}
					wave_sync();
				}
			}
			if (lane == 0)
			{
				t.needs_nn = needs ? 1 : 0;
				t.symmetry = symmetry;
				if (needs)
				{
					// each group owns the list segment of its games; a merged match launch fills the two players' lists (= groups 0 and 1 of 2)
					const int half = (E.match_merged && g >= E.n_games / 2) ? 1 : 0;
					const int first = E.match_merged ? half * (E.n_games / 2) : E.g0;
					const int idx = atomicAdd(&E.counters[E.nn_counter + half], 1);
					E.nn_list[static_cast<size_t>(first) * E.batch + idx] = g * E.batch + j;
					scheduled++;
				}
			}
			if (needs)
				queued++;
		}
		if (lane == 0)
			gs.nn_queued = queued;
		return scheduled;
	}

	/* NFIX: board size known at compile time (15, 20) or 0 for any size.  The solver divides and takes remainders by the board size
	 * all the time (cell <-> row, column); with a constant these are a multiply and a shift instead of ~40 instructions each. */
	/* FUSED: Search::select of the game runs in the same wave right before its solver (self-play and match pools; a tournament-search pool
	 * selects for all threads in one wave, k_select).  As two launches the select stage lasts as long as its slowest game (deep end-game
	 * paths, leak retries: measured 2.4 x the mean wave) while the other SIMDs idle; fused, a slow descent only delays its own game's solver
	 * and the launch ends with the yield rule as before.  The select stage's LDS (board, keys) aliases the threat lists, which the solver
	 * initialises afterwards. */
#ifndef AGX_SOLVE_WAVES
#define AGX_SOLVE_WAVES 1 /* waves per SIMD the register allocation of k_solve leaves room for: a pool of n games has n solver waves, one per SIMD at the
                             BASELINE pool size, and an uncapped allocation is the fastest single wave (k_search_spec is the kernel built for occupancy) */
#endif
	template<bool RENJU, int NFIX, bool FUSED>
	__global__ __launch_bounds__(64, AGX_SOLVE_WAVES) void k_solve(EngineDev E)
	{
		if (NFIX != 0)
		{
			E.n = NFIX;
			E.hw = NFIX * NFIX;
		}
		typedef SolverSharedT<(NFIX != 0) ? NFIX : MAXN> SH;
		__shared__ SH sh;
		const int g = E.g0 + blockIdx.x, lane = threadIdx.x;
		if (E.match_merged)
			use_player_search(E, g);
		if (FUSED)
		{
			static_assert(offsetof(SH, act) % 8 == 0 && offsetof(SH, frames) == offsetof(SH, act) + sizeof(sh.act) && offsetof(SH, ptype) == offsetof(SH, frames) + sizeof(sh.frames)
				&& offsetof(SH, threat) == offsetof(SH, ptype) + sizeof(sh.ptype) && offsetof(SH, items) == offsetof(SH, threat) + sizeof(sh.threat),
				"select-stage keys: 64-bit words over act + frames + ptype + threat + items (contiguous) and on over the per-solve scratch up to board");
			static_assert(offsetof(SH, board) - offsetof(SH, act) >= SH::SELECT_KEY_BYTES && offsetof(SH, board) > offsetof(SH, items) && sizeof(sh.lines) >= BWORDS * sizeof(u64),
				"select-stage LDS must fit");
			const GameState &sg = E.games[g];
			if (sg.active && sg.error == 0 && sg.outcome == 0 && !sg.grow_pending)
			{
				use_game_arenas(E, g);
				u64 *sel_keys = reinterpret_cast<u64*>(&sh.act[0]);
				u64 *sel_cboard = &sh.lines[0];
				uint8_t *sel_board = &sh.board[0];
				for (int i = lane; i < 3 * (1 + E.hw); i += 64)
					sel_keys[i] = E.nc_keys[i];
				if (!sg.solve_pending)
					select_batch(E, g, g, lane, sel_board, sel_cboard, sel_keys);
			}
			__threadfence(); // the tasks written by the select stage are read back below (other lanes, vector L1)
			__syncthreads();
		}
		GameState &gs = E.games[g];
		const bool idle = (!gs.active || gs.error != 0 || gs.outcome != 0 || E.games[E.shared_tree ? 0 : g].grow_pending != 0);
		const int n_tasks = idle ? 0 : gs.n_tasks;
		if (E.spec_on && !idle && gs.solve_pending)
		{ // (a speculative pool stepped with a serial launch: nothing of the last speculative launch may outlive this one)
			if (lane == 0)
				spec_discard_pending(E, g);
			__threadfence();
			__syncthreads();
		}
		if (n_tasks > 0)
			solver_load_threat_table(sh, E, lane);
		unsigned long long solver_nodes = 0;
		/*
		 * The tasks of a game are solved strictly in order (they share the game's transposition table), so a launch lasts as long as
		 * its slowest game.  To keep the other CUs from idling behind stragglers a game may YIELD between two tasks once
		 * yield_fraction of the launch's games have finished: it keeps its position in the batch, sits out this step's network /
		 * expand stages and resumes in the next launch.  Each game still sees exactly the same sequence of operations.
		 */
		// (match mode: about half of a group's trees wait for their opponents and count as done at once)
		const float fraction = E.match_mode ? 0.5f + 0.5f * E.yield_fraction : E.yield_fraction;
		const int threshold = (E.yield_fraction > 0.0f) ? static_cast<int>(fraction * gridDim.x) : 0x7FFFFFFF;
		int k = idle ? 0 : gs.solve_pos;
		bool yielded = false;
		const unsigned long long t_launch = (E.solve_time_ticks != 0ull) ? wall_clock64() : 0ull;
		for (; k < n_tasks; k++)
		{
			DTask &t = E.tasks[static_cast<size_t>(g) * E.batch + k];
			const int slot = g * E.batch + k;
			if ((t.flags & TF_BY_SOLVER) == 0)
			{
				if (E.solve_time_ticks != 0ull && lane == 0)
				{ // ab_search.setTimeLimit((endTime - getTime()) / (getBatchSize() - i)) (Search.cpp:175-180): this task's share of what is left
					const unsigned long long now = wall_clock64(), end = t_launch + E.solve_time_ticks;
					sh.time_deadline = now + ((end > now) ? (end - now) / static_cast<unsigned long long>(max(1, E.batch_limit - k)) : 0ull); // (the buffer's SIZE, not its fill: a partly filled batch gets the reference's smaller shares)
				}
				if (threshold != 0x7FFFFFFF && k > gs.solve_pos)
				{ // at least one task per launch is always solved, so every game makes progress
					int done = 0;
					if (lane == 0)
						done = __hip_atomic_load(&E.counters[E.yield_counter], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
					done = __builtin_amdgcn_readfirstlane(done);
					if (done >= threshold)
					{
						yielded = true;
						break;
					}
				}
				solve_task<RENJU>(sh, E, g, t, slot, gs.generation, lane, solver_nodes, g);
			}
		}
		if (yielded)
		{
			if (lane == 0)
			{
				gs.solve_pos = k;
				gs.solve_pending = 1;
				gs.stats[5] += solver_nodes;
			}
			return;
		}
		// Search::scheduleToNN (Search.cpp:184-199), once the whole batch has been solved
		const unsigned long long scheduled = idle ? 0ull : schedule_to_nn(sh, E, g, gs, n_tasks, lane);
		if (lane == 0)
		{
			if (!idle)
			{
				gs.solve_pos = 0;
				gs.solve_pending = 0;
				gs.stats[5] += solver_nodes;
				gs.stats[1] += scheduled;
			}
			atomicAdd(&E.counters[E.yield_counter], 1);
		}
	}


	/* ------------------------------------------------------------------------------------------------------------ */
	/*
	 * k_search_spec — Search::select + Search::solve + Search::scheduleToNN of a group of games as ONE launch of persistent waves
	 * (AgxEngineConfig.speculative_solver).
	 *
	 * Why: a game's leaves share its transposition table, so Search::solve (Search.cpp:159-183) handles them one after the other and
	 * k_solve gives a game one wave — 1024 waves on 1024 SIMDs, each a dependent chain that waits on LDS / L2 about half of the time with
	 * nobody to fill the gaps.  Measured on MI355X (profiles/r03_solver_occupancy.txt): the same solver code with three waves per SIMD
	 * delivers 2.6 x the solver nodes per second.  A pool of 1024 games only has that many waves if the ~6.6 leaves of a batch are solved at
	 * the same time, which is what this kernel does without changing any result:
	 *   1. every wave first takes games off a cursor and runs their select stage (select_batch, exactly as k_solve<.., FUSED>), then
	 *      queues one work item per leaf the solver has to look at;
	 *   2. the waves take items off the queue and solve them against the game's table AS IT WAS BEFORE THE BATCH: the table is only
	 *      read, every bucket a task touches is copied into the task's overlay (dev_solver.hpp) and modified there;
	 *   3. the wave that finishes a game's last leaf commits the batch in order: a task whose first-touch bucket copies still equal the
	 *      table has seen exactly what it would have seen in its turn, so its versions of the buckets it wrote are stored; otherwise (an
	 *      earlier leaf of the same batch changed a bucket it read: 3-5 % of the leaves) it is solved again right there, serially,
	 *      on the table itself.  Then the game's positions go to the network queue.
	 * No wave ever waits for another wave's result (the commit is done by whoever arrives last), the only spinning is on an empty queue
	 * while other waves are still selecting, and selects are themselves taken off a cursor by resident waves — so the launch cannot
	 * deadlock whatever the grid size.
	 */
	template<class SH>
	__device__ __forceinline__ void spec_flush(const SH &sh, SpecTask &h, int nodes, uint32_t flags0, float moves_left0, int lane)
	{
		const int cnt = sh.ov_count;
		for (int i = lane; i < cnt; i += 64)
			h.keys[i] = sh.ov_keys[i];
		if (lane < OV_CAP / 32)
			h.dirty[lane] = sh.ov_dirty[lane];
		if (lane == 0)
		{
			h.count = cnt;
			h.overflow = (sh.ov_overflow || sh.error == ERR_OVERLAY) ? 1 : 0;
			h.nodes = nodes;
			h.flags0 = flags0;
			h.moves_left0 = moves_left0;
			h.solved = 1;
		}
	}
	/* The commit of one game's batch, resumable: the wave that solved the game's last leaf walks the leaves in batch order from `k` on.
	 * Returns the index of a leaf that has to be solved again serially (the caller does that, straight on the table, and calls again with
	 * k + 1), -1 when the batch is committed and on the network queue, or -2 when the game was DEFERRED: a leaf needs its serial re-run while
	 * all but a few games of the launch are done (the yield rule of k_solve, AgxEngineConfig.solver_yield_fraction) — the leaves before it
	 * stay committed, the game sits out this step's network / expand stages and the next launch queues its remaining leaves again: the
	 * same operations one step later. */
#ifndef AGX_DEFER_ON_EMPTY_QUEUE
#define AGX_DEFER_ON_EMPTY_QUEUE 0 /* 1: a batch whose commit needs a serial re-run is also deferred once the launch's queue has run dry (spec_commit_game) */
#endif
	struct SpecCommit
	{
		int game, k, first; // first: where the game's batch began in THIS launch (0, or the solve_pos a deferred game came back with)
			bool table_changed;
			unsigned long long nodes, solved, reruns;
	};
	template<class SH>
	__device__ __forceinline__ int spec_commit_game(SH &sh, const EngineDev &E, SpecCommit &c, int lane, const int *c_done, int defer_threshold, const int *c_queue, int count)
	{ // c_queue: the launch's counters (select cursor, queue head, queue tail, games selected)
		const int g = c.game;
		GameState &gs = E.games[g];
		const int n_tasks = gs.n_tasks;
		u64 *tt = E.tt + static_cast<size_t>(g % E.tt_mod) * (E.tt_bucket_mask + 1ull) * 8ull; // (double-buffered search: both buffers of a thread use its one solver)
		for (int k = c.k; k < n_tasks; k++)
		{
			const int slot = g * E.batch + k;
			SpecTask &h = E.spec_tasks[slot];
			if (h.solved == 0)
				continue; // a proven edge: the solver never saw this task
			DTask &t = E.tasks[slot];
			const u64 *ov = E.spec_overlay + static_cast<size_t>(slot) * (SPEC_OV_CAP * 16);
			const int cnt = h.count;
			bool valid = (h.overflow == 0);
			{ // a header that does not describe an overlay (count or a bucket index out of range) can only mean that the solving wave's stores were
			  // not visible here: stop the game with an error instead of following a wild index
				bool bad = (cnt < 0 || cnt > SPEC_OV_CAP);
				for (int i = lane; !bad && i < cnt; i += 64)
					bad = static_cast<u64>(h.keys[i]) > E.tt_bucket_mask;
				if (__ballot(bad) != 0ull)
				{
					if (lane == 0)
					{
						gs.error = ERR_SPEC_STATE;
						h.solved = 0;
					}
					continue;
				}
			}
			if (valid && c.table_changed)
			{ // has any bucket this task looked at changed since the batch began?  Eight lanes per bucket.
				bool mismatch = false;
				for (int base = 0; base < cnt; base += 8)
				{
					const int p = base + (lane >> 3), w = lane & 7;
					if (p < cnt)
						mismatch = mismatch || (ov[p * 16 + w] != tt[8 * static_cast<u64>(h.keys[p]) + w]);
				}
				valid = (__ballot(mismatch) == 0ull);
			}
			if (!valid)
			{
				int done = 0;
				if (lane == 0)
					done = __hip_atomic_load(c_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
				// (like k_solve's rule: the first leaf of the launch is always finished — a game whose first pending leaf needs the re-run every time,
				//  e.g. one whose overlay overflows, would otherwise be deferred launch after launch with its speculative work thrown away)
#if AGX_DEFER_ON_EMPTY_QUEUE
				// ... or the launch has nothing left to hide a serial re-run behind: every game has queued its leaves and every leaf has been taken, so
				// the waves are leaving and a 1.1 ms re-run now only lengthens the launch (in-kernel trace, profiles/r05_search_launch_timeline.txt: the
				// games that end a launch are the ones whose commit began when the queue ran dry and needed one re-run)
				int dry = 0;
				if (lane == 0 && defer_threshold != 0x7FFFFFFF)
					dry = (__hip_atomic_load(c_queue + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= count
							&& __hip_atomic_load(c_queue + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= __hip_atomic_load(c_queue + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) ? 1 : 0;
				const bool defer = (__builtin_amdgcn_readfirstlane(done) >= defer_threshold || __builtin_amdgcn_readfirstlane(dry) != 0) && k > c.first;
#else
				const bool defer = __builtin_amdgcn_readfirstlane(done) >= defer_threshold && k > c.first;
#endif
				// forget the speculative result: of this leaf (it is solved again), or of this leaf and the ones behind it (deferred)
				for (int j = k; j < (defer ? n_tasks : k + 1); j++)
				{
					SpecTask &hj = E.spec_tasks[g * E.batch + j];
					if (hj.solved != 0 && lane == 0)
					{
						DTask &tj = E.tasks[g * E.batch + j];
						tj.flags = hj.flags0;
						tj.win = 0.0f;
						tj.draw = 0.0f;
						tj.moves_left = hj.moves_left0;
						hj.solved = 0;
					}
				}
				wave_sync();
				if (defer)
				{
					if (lane == 0)
					{
						gs.solve_pos = k;
						gs.solve_pending = 1;
						gs.stats[5] += c.nodes;
						gs.spec_stats[0] += c.solved;
						gs.spec_stats[1] += c.reruns;
						gs.spec_stats[2] += 1;
					}
					return -2;
				}
				// Search::solve's own order: this task again, on the table as the earlier tasks of the batch left it
				c.solved++;
				c.reruns++;
				c.table_changed = true;
				c.k = k + 1;
				return k;
			}
			bool any = false;
			for (int base = 0; base < cnt; base += 8)
			{
				const int p = base + (lane >> 3), w = lane & 7;
				if (p < cnt && ((h.dirty[p >> 5] >> (p & 31)) & 1u))
				{
					tt[8 * static_cast<u64>(h.keys[p]) + w] = ov[p * 16 + 8 + w];
					any = true;
				}
			}
			c.table_changed = c.table_changed || (__ballot(any) != 0ull);
			c.nodes += static_cast<unsigned long long>(h.nodes);
			c.solved++;
			if (lane == 0)
				h.solved = 0;
			wave_sync();
		}
		const unsigned long long scheduled = schedule_to_nn(sh, E, g, gs, n_tasks, lane);
		if (lane == 0)
		{
			gs.solve_pos = 0;
			gs.solve_pending = 0;
			gs.stats[5] += c.nodes;
			gs.stats[1] += scheduled;
			gs.spec_stats[0] += c.solved;
			gs.spec_stats[1] += c.reruns;
#ifdef AGX_SPEC_PROFILE
			E.spec_trace[4 * g + 3] = c.reruns * 16 + c.solved;
#endif
		}
		return -1;
	}

#ifdef AGX_SPEC_PROFILE /* developer builds: where the waves of k_search_spec spend their time (100 MHz wall clock ticks, summed over waves) */
#define SPEC_T(var) unsigned long long var = wall_clock64()
#define SPEC_ADD(k, v) do { if (lane == 0) atomicAdd(&E.spec_prof[k], static_cast<unsigned long long>(v)); } while (0)
#define SPEC_MAX(k, v) do { if (lane == 0) atomicMax(&E.spec_prof[k], static_cast<unsigned long long>(v)); } while (0)
/* per wave of the LAST launch: launch-relative ticks of its select phase's end and of its exit, leaves it solved, ticks it waited for items */
#define SPEC_WAVE_EXIT() do { if (lane == 0) { unsigned long long *w_ = E.spec_trace + 4 * (static_cast<size_t>(E.n_games) + E.spec_group * E.spec_waves + blockIdx.x); \
		w_[0] = t_selected; w_[1] = wall_clock64(); w_[2] = wave_solves; w_[3] = wave_waited; } } while (0)
#else
#define SPEC_T(var) do { } while (0)
#define SPEC_ADD(k, v) do { } while (0)
#define SPEC_MAX(k, v) do { } while (0)
#define SPEC_WAVE_EXIT() do { } while (0)
#endif
#ifndef AGX_SPEC_WAVES
#define AGX_SPEC_WAVES 3 /* waves per SIMD the register allocation of k_search_spec leaves room for on boards whose LDS state allows 9-12 waves per compute unit */
#endif
#ifndef AGX_SPEC_WAVES_15
#define AGX_SPEC_WAVES_15 4 /* ... and on 15x15 boards (10 240 bytes of LDS state: 16 waves per compute unit): 128 registers.  Measured (profiles/r05_search_variants_ab.txt,
                               boxes 11-12): the spills of the tighter allocation sit outside the solver's loops (69 scratch instructions in the whole kernel) and cost
                               nothing — at 12 waves per unit the 128-register kernel is as fast as the 168-register one —, and with 16 the launch is 8.6 % shorter */
#endif
	constexpr int spec_waves_per_simd(int nfix) { return (nfix == 15) ? AGX_SPEC_WAVES_15 : AGX_SPEC_WAVES; }
	/* MERGED: the launch covers both players' trees of a match pool (agx_engine_select_solve_match) and every game / work item takes its
	 * player's search settings (use_player_search).  A variant of its own, not a branch: this kernel runs at its register cap with scalar
	 * registers spilled, and the choice as a never-taken branch cost the self-play launch 0.4 % (DESIGN: "Players with their own search
	 * settings") — the other launches run the code they ran before. */
	template<bool RENJU, int NFIX, bool MERGED>
	__global__ __launch_bounds__(64, spec_waves_per_simd(NFIX)) void k_search_spec(EngineDev E, int count)
	{
		if (NFIX != 0)
		{
			E.n = NFIX;
			E.hw = NFIX * NFIX;
		}
		typedef SolverSharedT<(NFIX != 0) ? NFIX : MAXN> SH;
		__shared__ SH sh;
		const int lane = threadIdx.x;
		int *const c_select = E.counters + SPEC_COUNTER0 + 4 * E.spec_group, *const c_head = c_select + 1, *const c_tail = c_select + 2, *const c_selected = c_select + 3;
		int *const c_done = E.counters + E.yield_counter; // games of this launch whose batch is on the network queue (or that had nothing to do)
		const float fraction = E.match_mode ? 0.5f + 0.5f * E.yield_fraction : E.yield_fraction; // (match mode: half of the trees wait for their opponents)
		const int defer_threshold = (E.yield_fraction > 0.0f) ? static_cast<int>(fraction * count) : 0x7FFFFFFF;
		// Only the renju kernels park: their launches end with a few solves of several times the average length; on the other rules a launch ends with
		// commits and their re-runs (the yield rule's business), nothing was ever parked at this threshold (C2: 0-1 solves in 300 steps), and the code's
		// registers cost the launch 4 % (3.25 -> 3.40 ms).  For them the pointer below is a compile-time null and all of it folds away.
		constexpr bool SPEC_PARKS = RENJU;
		const ParkCtl park_ctl = { count, (E.park_fraction > 0.0f && count >= 4) ? static_cast<int>(E.park_fraction * count) : 0x7FFFFFFF };
		int *const items = E.spec_items + static_cast<size_t>(E.g0) * E.batch + static_cast<size_t>(E.spec_group) * SPEC_QUEUE_SLACK;
		const int item_cap = count * E.batch + SPEC_QUEUE_SLACK;
		const int area = E.n_games + E.spec_group * E.spec_waves + blockIdx.x; // this wave's spill areas (action stack, list / frame tails)

		/* ---- 1. select: games off a cursor ---- */
		static_assert(offsetof(SH, act) % 8 == 0 && offsetof(SH, frames) == offsetof(SH, act) + sizeof(sh.act) && offsetof(SH, ptype) == offsetof(SH, frames) + sizeof(sh.frames)
				&& offsetof(SH, threat) == offsetof(SH, ptype) + sizeof(sh.ptype) && offsetof(SH, items) == offsetof(SH, threat) + sizeof(sh.threat),
				"select-stage keys: 64-bit words over act + frames + ptype + threat + items (contiguous) and on over the per-solve scratch up to board");
		static_assert(offsetof(SH, board) - offsetof(SH, act) >= SH::SELECT_KEY_BYTES && offsetof(SH, board) > offsetof(SH, items) && sizeof(sh.lines) >= BWORDS * sizeof(u64),
				"select-stage LDS must fit");
		u64 *sel_keys = reinterpret_cast<u64*>(&sh.act[0]);
		bool keys_loaded = false;
		SPEC_T(t_begin);
		__builtin_amdgcn_s_setprio(3); // selects (and below: commits) are the launch's critical path, the speculative solves fill the SIMDs around them
		while (true)
		{
			int s = 0;
			if (lane == 0)
				s = atomicAdd(c_select, 1);
			s = __builtin_amdgcn_readfirstlane(s);
			if (s >= count)
				break;
			const int g = E.g0 + s;
			GameState &gs = E.games[g];
			// (tournament search: record g is a task buffer of tree 0, already filled by k_select — the threads take the tree in turn there; here
			//  its leaves are solved in parallel like any game's)
			const bool idle = (!gs.active || gs.error != 0 || gs.outcome != 0 || E.games[E.shared_tree ? 0 : g].grow_pending != 0);
			if (!idle)
			{
				if (!keys_loaded && !E.shared_tree)
				{
					for (int i = lane; i < 3 * (1 + E.hw); i += 64)
						sel_keys[i] = E.nc_keys[i];
					keys_loaded = true;
				}
				use_game_arenas(E, E.shared_tree ? 0 : g);
				if constexpr (MERGED)
					use_player_search(E, g);
				const int first = gs.solve_pending ? gs.solve_pos : 0; // a deferred game: no new descents, its batch goes on behind the committed leaves
				if (!gs.solve_pending && !E.shared_tree)
					select_batch(E, g, g, lane, &sh.board[0], &sh.lines[0], sel_keys);
				__threadfence(); // the tasks are read by other waves
				__syncthreads();
				const int n_tasks = gs.n_tasks;
				int n_items = 0;
				for (int k = first; k < n_tasks; k++)
					if ((E.tasks[static_cast<size_t>(g) * E.batch + k].flags & TF_BY_SOLVER) == 0)
						n_items++;
				if (n_items == 0)
				{ // nothing for the solver (proven edges only): the batch goes to the network queue at once
					const unsigned long long scheduled = schedule_to_nn(sh, E, g, gs, n_tasks, lane);
					if (lane == 0)
					{
						gs.stats[1] += scheduled;
						gs.solve_pos = 0;
						gs.solve_pending = 0;
						atomicAdd(c_done, 1);
					}
					keys_loaded = keys_loaded && !E.use_symmetries; // (symmetric features pass through sh.act, where the keys are)
				}
				else
				{
					if (lane == 0)
					{
						__hip_atomic_store(&E.spec_left[g], n_items, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
						__threadfence();
						const int base = atomicAdd(c_tail, n_items);
						int j = 0;
						for (int k = first; k < n_tasks; k++)
							if ((E.tasks[static_cast<size_t>(g) * E.batch + k].flags & TF_BY_SOLVER) == 0)
								__hip_atomic_store(&items[base + j++], (g * 16 + k) + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
					}
				}
			}
			if (idle && lane == 0)
			{
				if (gs.error != 0 && gs.solve_pending)
				{ // a game stopped for good with a batch in flight: its park buffers go back to the pool
					gs.solve_pending = 0;
					park_forget_game(E, g);
				}
				atomicAdd(c_done, 1);
			}
#ifdef AGX_SPEC_PROFILE
			if (lane == 0)
			{
				E.spec_trace[4 * g + 0] = wall_clock64();
				E.spec_trace[4 * g + 3] = 0;
			}
#endif
			if (lane == 0)
			{
				__threadfence();
				atomicAdd(c_selected, 1);
			}
			__syncthreads();
		}
		__syncthreads();

		__builtin_amdgcn_s_setprio(0);
		SPEC_T(t_selected);
		SPEC_ADD(0, t_selected - t_begin); // select phase, all waves (incl. the ones that found the cursor exhausted at once)
		SPEC_MAX(1, t_selected - t_begin); // the slowest wave's select phase
		/* ---- 2. + 3. solve the queued leaves, commit a game's batch when its last leaf is done ----
		 * One call site of the solver for both kinds of solves (speculative: against the task's overlay; re-run during a commit: straight on
		 * the table) — the solver is ~25 k instructions, a second inlined copy costs registers and instruction cache. */
		solver_load_threat_table(sh, E, lane);
		SpecCommit commit;
		commit.game = -1;
		SPEC_T(t_commit0);
#ifdef AGX_SPEC_PROFILE
		unsigned long long wave_solves = 0, wave_waited = 0;
#endif
		while (true)
		{
			int g, k;
			bool speculative;
			SPEC_T(t_pop);
			if (commit.game >= 0)
			{ // this wave is committing a game: go on until a leaf needs its serial re-run
				const int r = spec_commit_game(sh, E, commit, lane, c_done, defer_threshold, c_select, count);
				if (r < 0)
				{
					if (r == -1 && lane == 0)
						atomicAdd(c_done, 1);
#ifdef AGX_SPEC_PROFILE
					SPEC_T(t_c1);
					if (lane == 0)
					{
						E.spec_trace[4 * commit.game + 1] = t_commit0;
						E.spec_trace[4 * commit.game + 2] = t_c1;
					}
					SPEC_ADD(4, t_c1 - t_commit0); // commits incl. serial re-runs
					SPEC_MAX(5, t_c1 - t_commit0);
#endif
					commit.game = -1;
					__builtin_amdgcn_s_setprio(0);
					continue;
				}
				g = commit.game;
				k = r;
				speculative = false;
			}
			else
			{
				int i = 0;
				if (lane == 0)
					i = atomicAdd(c_head, 1);
				i = __builtin_amdgcn_readfirstlane(i);
				if (i >= item_cap)
				{
					SPEC_WAVE_EXIT();
					return;
				}
				int v = 0;
				if (lane == 0)
				{ // wait for queue slot i to be filled.  The waiting waves must not disturb the ones that still select (they are the critical path):
				  // each polls only its OWN slot (no shared hot spot), sleeps in between, and looks at the shared counters once in 32 polls
					for (int polls = 0;; polls++)
					{
						v = __hip_atomic_load(&items[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
						if (v != 0)
							break;
						if ((polls & 31) == 31 && __hip_atomic_load(c_selected, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= count)
						{ // every game has queued its leaves: the queue's length is final
							__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
							if (i >= __hip_atomic_load(c_tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
							{
								v = -1;
								break;
							}
						}
						if (polls > (1 << 22))
						{ // watchdog (seconds): a queue slot that never fills would hang the launch — report instead
							E.spec_watchdog[0] = 1;
							E.spec_watchdog[1] = i;
							E.spec_watchdog[2] = __hip_atomic_load(c_head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
							E.spec_watchdog[3] = __hip_atomic_load(c_tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
							E.spec_watchdog[4] = __hip_atomic_load(c_selected, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
							E.spec_watchdog[5] = count;
							E.spec_watchdog[6] = __hip_atomic_load(c_select, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
							E.games[E.g0].error = ERR_SPEC_STATE;
							v = -1;
							break;
						}
						__builtin_amdgcn_s_sleep(64);
					}
					if (v > 0)
						__hip_atomic_store(&items[i], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // empty again for the next launch
				}
				v = __builtin_amdgcn_readfirstlane(v);
				SPEC_T(t_got);
				SPEC_ADD(2, t_got - t_pop); // waiting for an item
#ifdef AGX_SPEC_PROFILE
				wave_waited += t_got - t_pop;
#endif
				if (v < 0)
				{
					SPEC_MAX(7, t_got - t_begin); // the last wave's exit = the launch
					SPEC_WAVE_EXIT();
					return;
				}
				__threadfence(); // (acquire: the task as its selecting wave wrote it)
				g = (v - 1) >> 4;
				k = (v - 1) & 15;
				speculative = true;
			}
			const int slot = g * E.batch + k;
			if constexpr (MERGED)
				use_player_search(E, g); // (the solver's node budget is the searching player's; the leaves of many games pass through one wave)
			DTask &t = E.tasks[slot];
			const uint32_t flags0 = t.flags;
			const float moves_left0 = t.moves_left;
			unsigned long long n1 = 0;
			SPEC_T(t_s0);
			const bool parked = solve_task<RENJU>(sh, E, g, t, slot, E.games[g].generation, lane, n1, area,
					speculative ? E.spec_overlay + static_cast<size_t>(slot) * (SPEC_OV_CAP * 16) : nullptr, (SPEC_PARKS && speculative) ? &park_ctl : nullptr);
			if (!speculative)
			{ // a re-run inside a commit: its result stands
				commit.nodes += n1;
				continue;
			}
			if (parked)
			{ // the solve goes on in the next launch (the queue is dry: this wave's next turn finds nothing and leaves)
				SPEC_T(t_parked);
				SPEC_ADD(3, t_parked - t_s0);
				continue;
			}
			spec_flush(sh, E.spec_tasks[slot], static_cast<int>(n1), flags0, moves_left0, lane);
			SPEC_T(t_solved);
			SPEC_ADD(3, t_solved - t_s0); // speculative solves
			SPEC_ADD(6, 1);
#ifdef AGX_SPEC_PROFILE
			wave_solves++;
#endif
			__threadfence(); // release: task results, features, overlay and its header
			int left = 0;
			if (lane == 0)
				left = __hip_atomic_fetch_add(&E.spec_left[g], -1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
			left = __builtin_amdgcn_readfirstlane(left);
			if (left == 1)
			{ // the last leaf of this game's batch: this wave commits it, in batch order (the loop's next turns)
				__threadfence();
				commit.game = g;
				commit.k = 0;
				commit.first = E.games[g].solve_pending ? E.games[g].solve_pos : 0;
				commit.table_changed = false;
				commit.nodes = commit.solved = commit.reruns = 0;
				__builtin_amdgcn_s_setprio(3);
#ifdef AGX_SPEC_PROFILE
				t_commit0 = wall_clock64();
#endif
			}
		}
	}

	/* ------------------------------------------------------------------------------------------------------------ */
#ifndef AGX_WIDE_BACKUP
#define AGX_WIDE_BACKUP 1 /* Tree::backup with all levels of a path in flight at once (k_expand); 0: level by level */
#endif
	template<bool MERGED> // (MERGED: as k_search_spec's)
	__global__ __launch_bounds__(64) void k_expand(EngineDev E)
	{
		__shared__ float e_prior[MAXHW], e_win[MAXHW], e_draw[MAXHW];
		__shared__ uint16_t e_move[MAXHW], e_score[MAXHW];
		__shared__ float sh_sum;
		__shared__ u64 sort_keys[512]; // prune_weak_moves with max_children: (score band, prior, original index) of every edge
		const int g0 = E.g0 + blockIdx.x, lane = threadIdx.x;
		const int tg = E.shared_tree ? 0 : g0; // the game that owns the tree; tournament search: every search thread works on tree 0
		GameState &gs = E.games[tg];
		if (!gs.active || gs.error != 0 || gs.outcome != 0 || (!E.shared_tree && gs.solve_pending) || gs.grow_pending == 1 || gs.grow_pending == 3)
			return;
		use_game_arenas(E, tg);
		if constexpr (MERGED)
			use_player_search(E, g0);
		DNode *nodes = nodes_of(E, tg, gs.arena);
		DEdge *edges = edges_of(E, tg, gs.arena);
		int *ht = ht_of(E, tg);
		const int n = E.n, hw = E.hw;
		const int first_lane = E.shared_tree ? E.grp_first : g0, last_lane = E.shared_tree ? E.grp_first + E.grp_count - 1 : g0;
		if (E.shared_tree && gs.grow_pending != 0 && gs.grow_owner != E.grp_first)
			return; // double-buffered search: the buffer whose expansion waits for larger arenas goes first, this one keeps its leaves one more turn
		{
			/*
			 * NodeCache::resize / ObjectPool growth (NodeCache.cpp:320-355, utils/ObjectPool.hpp:74-289) for flat arenas: BEFORE anything is
			 * modified, the batch's worst case (a node per task, every solver edge kept) is held against the game's arenas.  If it does not
			 * fit, the game asks for the next size class and sits this stage out with its batch untouched: k_arena_service / k_arena_copy
			 * move the tree into larger regions, select and solve skip the game in the next step, and this kernel then expands the SAME
			 * batch — the game performs exactly the same sequence of operations, one step later.
			 */
			int need_edges = gs.n_edges, need_nodes = gs.n_nodes;
			for (int lg = first_lane; lg <= last_lane; lg++)
			{
				const int lane_tasks = E.games[lg].n_tasks;
				need_nodes += lane_tasks;
				for (int k = 0; k < lane_tasks; k++)
					need_edges += E.tasks[static_cast<size_t>(lg) * E.batch + k].n_edges;
			}
			const bool fits = need_nodes <= E.node_cap && need_edges <= E.edge_cap && 2 * need_nodes <= E.ht_cap;
			if (!fits && gs.arena_class + 1 < ARENA_CLASSES && gs.grow_pending != 4)
			{ // (also straight after a growth that was not enough: one more class)
				if (lane == 0)
				{
					gs.grow_pending = 1;
					gs.grow_owner = E.grp_first;
				}
				return;
			}
			if (lane == 0)
				gs.grow_pending = 0; // 2 -> 0: grown; 4 -> 0: no heap space left (or the largest class reached): the exact per-node test below decides
		}
		const u64 lower = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
		// tournament search: the search threads take the tree in thread order, each expands its batch and backs it up (SearchThread.cpp:
		// 135-141); self-play: the one buffer of the game
		for (int g = first_lane; g <= last_lane; g++)
		{
		GameState &ls = E.games[g];
		const int n_tasks = ls.n_tasks;
		unsigned long long wasted = 0;

		for (int k = 0; k < n_tasks; k++)
		{
			DTask &t = E.tasks[static_cast<size_t>(g) * E.batch + k];
			const int slot = g * E.batch + k;
			uint32_t flags = t.flags;
			const uint32_t score = t.score;
			float win = t.win, draw = t.draw, moves_left = t.moves_left;
			const int path_len = t.path_len;
			const int sign = t.sign_to_move;
			if (t.needs_nn)
			{ // NNEvaluator::unpack_from_network (NNEvaluator.cpp:263-286), 'pv' network: the q / moves-left outputs are zero
				flags |= TF_BY_NETWORK;
				win = E.nn_value[3 * slot];
				draw = E.nn_value[3 * slot + 1];
				if (s_unproven(score))
					moves_left = 0.0f;
			}
			int n_e = t.n_edges;
			if ((flags & TF_SKIP_EDGE_GENERATION) == 0 && n_e > 0)
			{ // UnifiedGenerator::generate (EdgeGenerator.cpp:269-303)
				const bool by_network = (flags & TF_BY_NETWORK) != 0;
				const int inv_symmetry = inverse_symmetry(t.symmetry);
				for (int i = lane; i < n_e; i += 64)
				{ // initialize_edges (:88-127)
					const uint32_t mv = t.emove[i], sc = t.escore[i];
					int pr, pc; // the network saw the position under t.symmetry: task policy = apply_symmetry(output, inverse) (NNEvaluator.cpp:277-279)
					symmetry_source(inv_symmetry, n, (mv >> 2) & 127, (mv >> 9) & 127, pr, pc);
					const int cell = pr * n + pc;
					e_move[i] = static_cast<uint16_t>(mv);
					e_score[i] = static_cast<uint16_t>(sc);
					e_prior[i] = by_network ? E.nn_policy[static_cast<size_t>(slot) * hw + cell] : 0.0f;
					float w = 0.0f, d = 0.0f;
					if (!by_network && s_proven(sc))
						s_to_value(sc, w, d);
					if (by_network && E.has_q)
					{ // unpack_from_network overwrites every action value with the 'q' output (NNEvaluator.cpp:277-279)
						w = E.nn_q[(static_cast<size_t>(slot) * hw + cell) * 2];
						d = E.nn_q[(static_cast<size_t>(slot) * hw + cell) * 2 + 1];
					}
					e_win[i] = w;
					e_draw[i] = d;
				}
				if (E.policy_temperature != 1.0f)
				{ // initialize_edges with a temperature (:90-118)
					if (E.policy_temperature == 0.0f)
					{ // prior 1 where the policy holds its maximum over the WHOLE plane (maxValue(task.getPolicy())), 0 elsewhere
						uint32_t mx = 0; // non-negative floats order like their bit patterns
						if (by_network)
							for (int i = lane; i < hw; i += 64)
								mx = max(mx, __float_as_uint(E.nn_policy[static_cast<size_t>(slot) * hw + i]));
						mx = wave_max_u32(mx);
						for (int i = lane; i < n_e; i += 64)
							e_prior[i] = (__float_as_uint(e_prior[i]) == mx) ? 1.0f : 0.0f;
					}
					else
					{
						const float inv_t = 1.0f / E.policy_temperature;
						for (int i = lane; i < n_e; i += 64)
						{
							const float p = e_prior[i];
							e_prior[i] = (p > 0.0f) ? static_cast<float>(det_exp(det_log(static_cast<double>(p)) * static_cast<double>(inv_t))) : 0.0f;
						}
					}
				}
				__syncthreads();
				if ((path_len > 0 || E.prune_root) && s_proven(score))
				{ // the root is exempt in self-play only (forceExpandRoot: GameGenerator.cpp:183-184, Player.cpp:111); prune_weak_moves, proven branch (:55-68): keep the best-scored edges in their original order
					uint32_t best = s_loss_in(0);
					for (int i = lane; i < n_e; i += 64)
						best = max(best, static_cast<uint32_t>(e_score[i]));
					best = wave_max_u32(best);
					int kept = 0;
					for (int base = 0; base < n_e; base += 64)
					{
						const int i = base + lane;
						const bool keep = (i < n_e) && (e_score[i] == best);
						const uint16_t mv = (i < n_e) ? e_move[i] : 0, sc = (i < n_e) ? e_score[i] : 0;
						const float p = (i < n_e) ? e_prior[i] : 0.0f, w = (i < n_e) ? e_win[i] : 0.0f, d = (i < n_e) ? e_draw[i] : 0.0f;
						const u64 m = __ballot(keep);
						__syncthreads();
						if (keep)
						{
							const int dst = kept + __popcll(m & lower);
							e_move[dst] = mv;
							e_score[dst] = sc;
							e_prior[dst] = p;
							e_win[dst] = w;
							e_draw[dst] = d;
						}
						kept += __popcll(m);
						__syncthreads();
					}
					n_e = kept;
				}
				else if ((path_len > 0 || E.prune_root) && n_e > E.max_children && (flags & TF_MUST_DEFEND) == 0)
				{ // prune_weak_moves, unproven branch (:69-83): the max_children best edges by EdgeComparator<MaxPolicyPrior>
				  // (Edge.hpp:156-172: proven scores first, then prior), then those whose prior reaches threshold * (their prior sum).
				  // std::partial_sort leaves the order of equal keys unspecified; here (and in the oracle) equal keys keep edge order.
					for (int i = lane; i < 512; i += 64)
					{
						u64 key = 0;
						if (i < n_e)
						{
							const uint32_t sc = e_score[i];
							const u64 band = s_proven(sc) ? sc : 0x4000u; // every unproven score shares one band between DRAW and WIN
							key = (band << 48) | (static_cast<u64>(__float_as_uint(e_prior[i])) << 16) | static_cast<u64>(0xFFFF - i);
						}
						sort_keys[i] = key;
					}
					__syncthreads();
					for (int k = 2; k <= 512; k <<= 1)
						for (int j = k >> 1; j > 0; j >>= 1)
						{ // bitonic network, descending
							for (int t = lane; t < 256; t += 64)
							{
								const int lo = ((t / j) * 2 * j) + (t % j), hi = lo + j;
								const u64 a = sort_keys[lo], b = sort_keys[hi];
								const bool descending = ((lo & k) == 0);
								if ((a < b) == descending)
								{
									sort_keys[lo] = b;
									sort_keys[hi] = a;
								}
							}
							__syncthreads();
						}
					const int K = E.max_children;
					if (lane == 0)
					{
						float sum = 0.0f;
						for (int r = 0; r < K; r++)
							sum += e_prior[0xFFFF - static_cast<int>(sort_keys[r] & 0xFFFFu)];
						sh_sum = E.expansion_threshold * sum;
					}
					__syncthreads();
					const float threshold = sh_sum;
					// gather the survivors (a prefix of the sorted list) into registers, then overwrite the edge arrays
					uint16_t g_mv[7], g_sc[7];
					float g_p[7], g_w[7], g_d[7];
					int kept = 0;
#pragma unroll
					for (int c = 0; c < 7; c++)
					{
						const int r = c * 64 + lane;
						const int src = (r < K) ? (0xFFFF - static_cast<int>(sort_keys[r] & 0xFFFFu)) : 0;
						g_mv[c] = e_move[src];
						g_sc[c] = e_score[src];
						g_p[c] = e_prior[src];
						g_w[c] = e_win[src];
						g_d[c] = e_draw[src];
						kept += __popcll(__ballot(r < K && g_p[c] >= threshold));
					}
					__syncthreads();
#pragma unroll
					for (int c = 0; c < 7; c++)
					{
						const int r = c * 64 + lane;
						if (r < kept)
						{
							e_move[r] = g_mv[c];
							e_score[r] = g_sc[c];
							e_prior[r] = g_p[c];
							e_win[r] = g_w[c];
							e_draw[r] = g_d[c];
						}
					}
					__syncthreads();
					n_e = kept;
				}
				// renormalize_policy (:23-40): the sum runs in edge order in fp32, exactly like the reference.  (As a loop of one lane over LDS every
				// addend was a full LDS round trip; now 64 priors travel into registers at once and the additions take them lane by lane: the same
				// additions in the same order, one v_readlane apiece, on every lane alike.)
				float sum = 0.0f;
				for (int base = 0; base < n_e; base += 64)
				{
					const int mine_i = __float_as_int((base + lane < n_e) ? e_prior[base + lane] : 0.0f);
					const int m = min(64, n_e - base);
					int j = 0;
					for (; j + 4 <= m; j += 4)
					{
						sum += __int_as_float(__builtin_amdgcn_readlane(mine_i, j));
						sum += __int_as_float(__builtin_amdgcn_readlane(mine_i, j + 1));
						sum += __int_as_float(__builtin_amdgcn_readlane(mine_i, j + 2));
						sum += __int_as_float(__builtin_amdgcn_readlane(mine_i, j + 3));
					}
					for (; j < m; j++)
						sum += __int_as_float(__builtin_amdgcn_readlane(mine_i, j));
				}
				if (sum == 0.0f)
				{
					const float u = 1.0f / n_e;
					for (int i = lane; i < n_e; i += 64)
						e_prior[i] = u;
				}
				else
				{
					const float inv = 1.0f / sum;
					for (int i = lane; i < n_e; i += 64)
						e_prior[i] = e_prior[i] * inv;
				}
				__syncthreads();
			}
			else
				n_e = 0;

			// ---- Tree::expand (Tree.cpp:257-298) ----
			int final_node = t.final_node;
			if (n_e > 0)
			{
				const int found = cache_seek(E, nodes, ht, t.hash, t.cboard, sign, lane);
				if (found < 0)
				{
					const int nid = gs.n_nodes, ebeg = gs.n_edges;
					if (nid >= E.node_cap || ebeg + n_e > E.edge_cap || 2 * (nid + 1) > E.ht_cap)
					{
						if (lane == 0)
							gs.error = (nid >= E.node_cap) ? ERR_NODE_CAPACITY : ((ebeg + n_e > E.edge_cap) ? ERR_EDGE_CAPACITY : ERR_HASH_TABLE);
						__syncthreads();
						return;
					}
					uint32_t max_score = 0;
					for (int i = lane; i < n_e; i += 64)
					{
						DEdge e;
						e.prior = e_prior[i];
						e.win = e_win[i];
						e.draw = e_draw[i];
						e.visits = 0;
						e.move = e_move[i];
						e.score = e_score[i];
						e.flag_vl = 0;
						e.pad = 0;
						edges[ebeg + i] = e;
						max_score = max(max_score, static_cast<uint32_t>(e_score[i]));
					}
					max_score = wave_max_u32(max_score);
					if (lane < BWORDS)
						nodes[nid].cboard[lane] = t.cboard[lane];
					if (lane == 0)
					{
						DNode &nd = nodes[nid];
						nd.edge_begin = ebeg;
						nd.n_edges = static_cast<int16_t>(n_e);
						nd.depth = static_cast<int16_t>(gs.n_moves + path_len);
						nd.vl = 0;
						nd.sign_to_move = static_cast<uint8_t>(sign);
						nd.pad8 = 0;
						nd.hash = t.hash;
						// updateValue from the cleared state (Node.hpp:268-274): visits 0 -> 1
						nd.visits = 1;
						const float tmp = static_cast<float>(1.0 / 1);
						float w = 0.0f + (win - 0.0f) * tmp, d = 0.0f + (draw - 0.0f) * tmp;
						nd.win = fmaxf(0.0f, fminf(1.0f, w));
						nd.draw = fmaxf(0.0f, fminf(1.0f, d));
						nd.moves_left = 0.0f + (moves_left - 0.0f) / 1;
						uint16_t nf = 0;
						if ((flags & TF_MUST_DEFEND) || (n_e + nd.depth) == hw)
							nf |= 4;
						nf |= ((flags & TF_STATICALLY_SOLVED) ? 8 : 0) | ((flags & TF_RECURSIVELY_SOLVED) ? 16 : 0) | ((flags & TF_MUST_DEFEND) ? 32 : 0);
						if (path_len == 0)
							nf |= 2;
						nd.flags = nf;
						nd.score = static_cast<uint16_t>(s_unknown(0));
						if ((nf & 4) || s_win(max_score) || s_unproven(max_score))
							nd.score = static_cast<uint16_t>(max_score);
						cache_insert(E, ht, t.hash, nid);
						gs.n_nodes = nid + 1;
						gs.n_edges = ebeg + n_e;
						if (path_len == 0)
							gs.root = nid;
					}
					final_node = nid;
					__syncthreads();
				}
				else
				{
					final_node = found;
					wasted++;
					if (path_len > 0)
					{
						const DEdge le = edges[t.path_edge[path_len - 1]];
						if (has_leak(E, le, true, nodes[found].score, nodes[found].win, nodes[found].draw))
							correct_information_leak(nodes, edges, t, path_len, final_node, lane);
					}
				}
			}

			if (lane == 0)
			{ // keep what the backup pass needs (Search::expand runs over ALL tasks before Search::backup, Search.cpp:214-232)
				t.final_node = final_node;
				t.win = win;
				t.draw = draw;
				t.moves_left = moves_left;
				t.flags = flags;
			}
			__syncthreads();
		}

		for (int k = 0; k < n_tasks; k++)
		{
			DTask &t = E.tasks[static_cast<size_t>(g) * E.batch + k];
			const float win = t.win, draw = t.draw;
			const int path_len = t.path_len, sign = t.sign_to_move, final_node = t.final_node;
			// ---- Tree::backup (Tree.cpp:299-351) ----
			// Every lane carries the same arithmetic (lane 0 stores it): a level costs one round trip for its node head + edge and one
			// for the score scan; the child's score travels up in a register instead of being read back.
			float ml = t.moves_left;
			bool have_child = final_node >= 0;
			uint32_t child_score = have_child ? nodes[final_node].score : 0u;
#if AGX_WIDE_BACKUP
			if (path_len <= 64)
			{ /* All levels of the path at once.  Level by level (below) a leaf costs two DEPENDENT round trips to HBM per level — the node head + edge,
			   * then the scan of the node's edge scores — and a path is ~8 levels deep: the expand stage was that chain (75 % of its wave cycles parked
			   * at s_waitcnt).  Nothing in a level's running means depends on another level (a position occurs once on a path), only the proven SCORE
			   * travels upwards: lane i takes level i — head, edge and value update —, the score scans of up to eight levels are requested together,
			   * and the score chain then runs over registers.  The arithmetic of every level is the serial loop's, operation for operation. */
				const bool mine = lane < path_len;
				const int node = mine ? t.path_node[lane] : 0, e = mine ? t.path_edge[lane] : 0;
				DNode nd;
				node_head(nd, nodes[node]);
				DEdge ed = edges[e];
				float ml_i = ml; // the serial loop adds 1.0f per level on its way up: the same additions, not one multiple
				for (int k = path_len - 1; k > lane; k--)
					ml_i += 1.0f;
				float vw = win, vd = draw;
				if (nd.sign_to_move != sign)
				{
					vw = 1.0f - (win + draw);
					vd = draw;
				}
				nd.visits++;
				const float tn = static_cast<float>(1.0 / nd.visits);
				nd.win = fmaxf(0.0f, fminf(1.0f, nd.win + (vw - nd.win) * tn));
				nd.draw = fmaxf(0.0f, fminf(1.0f, nd.draw + (vd - nd.draw) * tn));
				ed.visits++;
				const float te = 1.0f / ed.visits;
				ed.win = fmaxf(0.0f, fminf(1.0f, ed.win + (vw - ed.win) * te));
				ed.draw = fmaxf(0.0f, fminf(1.0f, ed.draw + (vd - ed.draw) * te));
				nd.moves_left += (ml_i - nd.moves_left) / nd.visits;
				nd.vl--;
				ed.flag_vl = static_cast<uint16_t>(((ed.flag_vl & 0x7FFF) - 1) & 0x7FFF);
				// the largest score among the OTHER edges of every level's node
				uint32_t others = 0;
				constexpr int LEVELS = 8, LOADS = (MAXHW + 63) / 64;
				for (int base = 0; base < path_len; base += LEVELS)
				{
					uint32_t sc[LEVELS][LOADS];
#pragma unroll
					for (int u = 0; u < LEVELS; u++)
					{
						const int lv = min(base + u, path_len - 1);
						const int eb = __builtin_amdgcn_readlane(nd.edge_begin, __builtin_amdgcn_readfirstlane(lv));
						const int ne = __builtin_amdgcn_readlane(static_cast<int>(nd.n_edges), __builtin_amdgcn_readfirstlane(lv));
						const int ee = __builtin_amdgcn_readlane(e, __builtin_amdgcn_readfirstlane(lv));
#pragma unroll
						for (int jj = 0; jj < LOADS; jj++)
						{
							const int j = lane + 64 * jj;
							sc[u][jj] = (base + u < path_len && j < ne && eb + j != ee) ? static_cast<uint32_t>(edges[eb + j].score) : 0u;
						}
					}
#pragma unroll
					for (int u = 0; u < LEVELS; u++)
					{
						uint32_t m = 0;
#pragma unroll
						for (int jj = 0; jj < LOADS; jj++)
							m = max(m, sc[u][jj]);
						m = wave_max_u32(m);
						if (lane == base + u)
							others = m;
					}
				}
				// the score chain, leaf to root, on registers
				for (int i = path_len - 1; i >= 0; i--)
				{
					const int li = __builtin_amdgcn_readfirstlane(i);
					uint32_t new_score = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(ed.score), li));
					if (have_child)
						new_score = s_invert_up(child_score);
					const uint32_t result = max(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(others), li)), new_score);
					const uint32_t level_flags = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(nd.flags), li));
					uint32_t node_score = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(nd.score), li));
					if (((level_flags & 4u) != 0u) || s_win(result) || s_unproven(result))
						node_score = result;
					if (lane == i)
					{
						ed.score = static_cast<uint16_t>(new_score);
						nd.score = static_cast<uint16_t>(node_score);
					}
					child_score = node_score;
					have_child = true;
				}
				if (mine)
				{
					DNode &dn = nodes[node];
					dn.visits = nd.visits;
					dn.win = nd.win;
					dn.draw = nd.draw;
					dn.moves_left = nd.moves_left;
					dn.vl = nd.vl;
					dn.score = nd.score;
					edges[e] = ed;
				}
				__syncthreads();
				continue;
			}
#endif
			for (int i = path_len - 1; i >= 0; i--)
			{
				const int node = t.path_node[i], e = t.path_edge[i];
				DNode nd;
				node_head(nd, nodes[node]);
				DEdge ed = edges[e];
				float vw = win, vd = draw;
				if (nd.sign_to_move != sign)
				{
					vw = 1.0f - (win + draw);
					vd = draw;
				}
				nd.visits++;
				const float tn = static_cast<float>(1.0 / nd.visits); // Node::updateValue: reciprocal in double, narrowed
				nd.win = fmaxf(0.0f, fminf(1.0f, nd.win + (vw - nd.win) * tn));
				nd.draw = fmaxf(0.0f, fminf(1.0f, nd.draw + (vd - nd.draw) * tn));
				ed.visits++;
				const float te = 1.0f / ed.visits; // Edge::updateValue: fp32 reciprocal
				ed.win = fmaxf(0.0f, fminf(1.0f, ed.win + (vw - ed.win) * te));
				ed.draw = fmaxf(0.0f, fminf(1.0f, ed.draw + (vd - ed.draw) * te));
				nd.moves_left += (ml - nd.moves_left) / nd.visits;
				uint32_t new_score = ed.score;
				if (have_child)
					new_score = s_invert_up(child_score);
				ed.score = static_cast<uint16_t>(new_score);
				nd.vl--;
				ed.flag_vl = static_cast<uint16_t>(((ed.flag_vl & 0x7FFF) - 1) & 0x7FFF);
				// update_score(Node*) (Tree.cpp:93-104) on the registers
				uint32_t result = 0;
				for (int j = lane; j < nd.n_edges; j += 64)
					result = max(result, (nd.edge_begin + j == e) ? new_score : static_cast<uint32_t>(edges[nd.edge_begin + j].score));
				result = wave_max_u32(result);
				if (((nd.flags & 4) != 0) || s_win(result) || s_unproven(result))
					nd.score = static_cast<uint16_t>(result);
				if (lane == 0)
				{
					DNode &dn = nodes[node];
					dn.visits = nd.visits;
					dn.win = nd.win;
					dn.draw = nd.draw;
					dn.moves_left = nd.moves_left;
					dn.vl = nd.vl;
					dn.score = nd.score;
					edges[e] = ed;
				}
				child_score = nd.score;
				have_child = true;
				ml += 1.0f;
			}
			__syncthreads();
		}

		if (lane == 0)
		{
			ls.stats[0] += n_tasks;
			ls.stats[4] += wasted;
			ls.n_tasks = 0;
		}
		__syncthreads();
		} // search threads
		if (lane == 0)
		{
			gs.stats[10] = max(gs.stats[10], static_cast<unsigned long long>(gs.n_nodes));
			gs.stats[11] = max(gs.stats[11], static_cast<unsigned long long>(gs.n_edges));
			// move rule (GameGenerator.cpp:97-103, utils/misc.cpp:171-179)
			if (gs.root >= 0)
			{
				const DNode &r = nodes[gs.root];
				const float reduction = fmaxf(0.0f, fminf(1.0f, (r.draw - 0.75f) / (1.0f - 0.75f)));
				const int simulations = static_cast<int>(E.max_sims - reduction * (E.max_sims - 50));
				gs.need_move = (r.visits > simulations || s_proven(r.score)) ? 1 : 0;
			}
		}
	}

	/* ------------------------------------------------------------------------------------------------------------ */
	template<int TPB = 256>
	__device__ void block_reduce_xor(u64 &v, u64 *scratch, int tid)
	{ // scratch: TPB / 64 words
		v = wave_reduce_xor64(v);
		__syncthreads();
		if ((tid & 63) == 0)
			scratch[tid >> 6] = v;
		__syncthreads();
		v = 0;
		for (int w = 0; w < TPB / 64; w++)
			v ^= scratch[w];
		__syncthreads();
	}
	__device__ void clear_solver_table(const EngineDev &E, int g, int tid)
	{ // AlphaBetaSearch::clear (SharedHashTable.hpp:137-140)
		ulonglong2 *tt = reinterpret_cast<ulonglong2*>(E.tt + static_cast<size_t>(g % E.tt_mod) * (E.tt_bucket_mask + 1ull) * 8ull);
		const size_t entries = (E.tt_bucket_mask + 1ull) * 4ull;
		ulonglong2 empty;
		empty.x = 0ull;
		empty.y = tt_pack(0, 0, s_unknown(0), 0);
		for (size_t i = tid; i < entries; i += 256)
			tt[i] = empty;
	}
	__device__ void clear_tree_and_table(const EngineDev &E, int g, int tid)
	{ // Tree::clear + AlphaBetaSearch::clear (GameGenerator.cpp:52-53)
		int *ht = ht_of(E, g);
		for (int i = tid; i < E.games[g].ht_cap; i += 256)
			ht[i] = 0;
		clear_solver_table(E, g, tid);
	}
	/* loads opening `id` into game g: Game::loadOpening + prepare_search on an empty tree (GameGenerator.cpp:48-77,174-185) */
	__device__ void begin_game(const EngineDev &E, int g, int id, int tid, u64 *scratch, bool tables_cleared = false, const uint16_t *saved_moves = nullptr, int saved_count = 0)
	{ // saved_moves: a game in flight restored from a checkpoint (GameGenerator::load, GameGenerator.cpp:131-141) — its moves so far instead of opening `id`
		GameState &gs = E.games[g];
		if (!tables_cleared)
			clear_tree_and_table(E, g, tid);
		for (int i = tid; i < E.hw; i += 256)
			gs.board[i] = 0;
		if (tid < BWORDS)
			gs.cboard[tid] = 0;
		__syncthreads();
		const uint16_t *op = (saved_moves != nullptr) ? saved_moves - 1 : E.openings + static_cast<size_t>(id) * OPENING_CAP;
		const int count = (saved_moves != nullptr) ? saved_count : op[0];
		if (tid == 0)
		{
			int sign = 1;
			for (int i = 0; i < count; i++)
			{
				const uint32_t mv = op[1 + i];
				const int cell = ((mv >> 2) & 127) * E.n + ((mv >> 9) & 127);
				gs.board[cell] = static_cast<uint8_t>(mv & 3);
				gs.cboard[cell >> 5] |= static_cast<u64>(mv & 3) << (2 * (cell & 31));
				gs.moves[i] = static_cast<uint16_t>(mv);
				sign = 3 - static_cast<int>(mv & 3);
			}
			gs.sign_to_move = sign;
			gs.n_moves = count;
			gs.outcome = 0;
			gs.root = -1;
			gs.n_nodes = 0;
			gs.n_edges = 0;
			gs.n_tasks = 0;
			gs.need_move = 0;
			gs.solve_pos = 0;
			gs.solve_pending = 0;
			park_forget_game(E, g);
			gs.max_depth = 0;
			gs.nn_queued = 0;
			gs.restart_id = 0;
			gs.noise_ready = 0;
			gs.generation = (gs.generation + 1) % 64; // prepare_search -> increaseGeneration
			gs.opening_id = id;
			gs.active = 1;
		}
		__syncthreads();
		u64 h = 0;
		for (int i = tid; i < E.hw; i += 256)
			h ^= E.nc_keys[3 + 3 * i + gs.board[i]];
		block_reduce_xor(h, scratch, tid);
		if (tid == 0)
			gs.root_hash = h ^ E.nc_keys[gs.sign_to_move];
		__syncthreads();
	}

	/*
	 * prepare_search / Player::setBoard for tree t on the position in its GameState (GameGenerator.cpp:174-185, Player.cpp:98-110):
	 * NodeCache::cleanup (NodeCache.cpp:221-249) as keep-test + prefix sum + copy to the other arena, Search::setBoard
	 * (increaseGeneration), Tree::setBoard (root = seek(new board), Tree.cpp:146-149).  Whole workgroup of TPB threads.
	 * DropRoot (set-board with forceRemoveRootNode, Tree.cpp:145-147): the keep test also drops the node of the new position itself, so the
	 * root is absent afterwards; nothing points at it (children are found by hash) and the table is rebuilt from the kept nodes.
	 */
	template<int TPB, bool DropRoot = false>
	__device__ void rebase_tree(const EngineDev &E0, int t, int tid, u64 *scratch, int *scan_nodes, int *scan_edges)
	{
		EngineDev E = E0;
		use_game_arenas(E, t); // (in match mode t is the partner's tree, not the workgroup's own game)
		GameState &gs = E.games[t];
		const int lane = tid & 63, wave = tid >> 6;
		DNode *nodes = nodes_of(E, t, gs.arena);
		DEdge *edges = edges_of(E, t, gs.arena);
		DNode *dst_nodes = nodes_of(E, t, gs.arena ^ 1);
		DEdge *dst_edges = edges_of(E, t, gs.arena ^ 1);
		int *ht = ht_of(E, t);
		for (int i = tid; i < E.ht_cap; i += TPB)
			ht[i] = 0;
		const int total = gs.n_nodes;
		int node_base = 0, edge_base = 0;
		u64 drop_hash = 0;
		if constexpr (DropRoot)
		{ // the new root's key, before the scan
			for (int i = tid; i < E.hw; i += TPB)
				drop_hash ^= E.nc_keys[3 + 3 * i + gs.board[i]];
			block_reduce_xor<TPB>(drop_hash, scratch, tid);
			drop_hash ^= E.nc_keys[gs.sign_to_move];
		}
		__syncthreads();
		for (int base = 0; base < total; base += TPB)
		{
			const int i = base + tid;
			int keep = 0, ne = 0;
			if (i < total)
			{
				keep = 1;
				u64 differs = 0;
				for (int w = 0; w < BWORDS; w++)
				{ // isTransitionPossibleFrom (NodeCache.cpp:95-115): every stone of the new position must be present
					const u64 from = gs.cboard[w], to = nodes[i].cboard[w];
					if (((from ^ to) & from) != 0)
						keep = 0;
					differs |= from ^ to;
				}
				if constexpr (DropRoot)
				{ // NodeCache::remove(newBoard, signToMove): same key, same side to move, same board
					if (differs == 0 && nodes[i].hash == drop_hash && nodes[i].sign_to_move == gs.sign_to_move)
						keep = 0;
				}
				ne = keep ? nodes[i].n_edges : 0;
			}
			scan_nodes[tid] = keep;
			scan_edges[tid] = ne;
			__syncthreads();
			for (int o = 1; o < TPB; o <<= 1)
			{ // inclusive Hillis-Steele scan
				const int a = (tid >= o) ? scan_nodes[tid - o] : 0, b = (tid >= o) ? scan_edges[tid - o] : 0;
				__syncthreads();
				scan_nodes[tid] += a;
				scan_edges[tid] += b;
				__syncthreads();
			}
			int cp_src = 0, cp_dst = 0;
			if (keep)
			{
				const int ni = node_base + scan_nodes[tid] - 1, eb = edge_base + scan_edges[tid] - ne;
				DNode nd = nodes[i];
				cp_src = nd.edge_begin;
				cp_dst = eb;
				nd.edge_begin = eb;
				dst_nodes[ni] = nd;
				// re-insert (atomic linear probing; slot order is irrelevant to lookups)
				const int mask = E.ht_cap - 1;
				int slot = static_cast<int>(nd.hash & static_cast<u64>(mask));
				while (atomicCAS(&ht[slot], 0, ni + 1) != 0)
					slot = (slot + 1) & mask;
			}
			// the edges: one node per wave at a time, its records copied by 64 lanes as 8-byte words (coalesced; 24-byte records of
			// per-thread copies touch three times the cache lines).  The node's (source, destination, count) come from its thread by
			// v_readlane — node k of the chunk belongs to lane k % 64 of wave k / 64.
			{
				const u64 *src64 = reinterpret_cast<const u64*>(edges);
				u64 *dst64 = reinterpret_cast<u64*>(dst_edges);
				for (int k = 0; k < 64; k++)
				{
					const int words = 3 * __builtin_amdgcn_readlane(ne, k);
					if (words == 0)
						continue;
					const size_t so = 3 * static_cast<size_t>(__builtin_amdgcn_readlane(cp_src, k)), dof = 3 * static_cast<size_t>(__builtin_amdgcn_readlane(cp_dst, k));
					for (int d = lane; d < words; d += 256)
					{
						const u64 w0 = src64[so + d];
						const u64 w1 = (d + 64 < words) ? src64[so + d + 64] : 0ull;
						const u64 w2 = (d + 128 < words) ? src64[so + d + 128] : 0ull;
						const u64 w3 = (d + 192 < words) ? src64[so + d + 192] : 0ull;
						dst64[dof + d] = w0;
						if (d + 64 < words)
							dst64[dof + d + 64] = w1;
						if (d + 128 < words)
							dst64[dof + d + 128] = w2;
						if (d + 192 < words)
							dst64[dof + d + 192] = w3;
					}
				}
			}
			node_base += scan_nodes[TPB - 1];
			edge_base += scan_edges[TPB - 1];
			__syncthreads();
		}
		u64 h = 0;
		for (int i = tid; i < E.hw; i += TPB)
			h ^= E.nc_keys[3 + 3 * i + gs.board[i]];
		block_reduce_xor<TPB>(h, scratch, tid);
		if (tid == 0)
		{
			gs.root_hash = h ^ E.nc_keys[gs.sign_to_move];
			gs.n_nodes = node_base;
			gs.n_edges = edge_base;
			gs.arena ^= 1;
			gs.generation = (gs.generation + 1) % 64;
			gs.max_depth = 0; // Tree.cpp:150
		}
		__syncthreads();
		if (wave == 0)
		{ // Tree::setBoard: root = seek(new board) (Tree.cpp:146-149)
			const int found = cache_seek(E, dst_nodes, ht, gs.root_hash, gs.cboard, gs.sign_to_move, lane);
			if (lane == 0)
			{
				gs.root = found;
				if (found >= 0)
					dst_nodes[found].flags |= 2;
			}
		}
		__syncthreads();
	}

	__global__ __launch_bounds__(256) void k_begin(EngineDev E)
	{
		__shared__ u64 scratch[4];
		const int g = blockIdx.x, tid = threadIdx.x;
		GameState &gs = E.games[g];
		__shared__ int sh_id;
		if (tid == 0)
		{
			sh_id = E.shared_tree ? 0 : g; // the first wave of games takes openings 0..n_games-1 in order; counters[1] is preset to n_games
			                               // (tournament search: every search thread starts on opening 0, counters[1] is preset to 1)
			gs.generation = 0;
			gs.error = 0;
			gs.games_done = 0;
			gs.arena = 0;
			for (int i = 0; i < 12; i++)
				gs.stats[i] = 0;
		}
		__syncthreads();
		if (E.match_mode)
		{ // every pair starts through k_assign_openings / k_match_restart: empty trees, the first players' trees ask for openings
			clear_tree_and_table(E, g, tid);
			if (tid == 0)
			{
				gs.active = 0;
				gs.root = -1;
				gs.n_nodes = 0;
				gs.n_edges = 0;
				gs.n_tasks = 0;
				gs.need_move = 0;
				gs.solve_pos = 0;
				gs.solve_pending = 0;
				park_forget_game(E, g);
				gs.outcome = 0;
				gs.n_moves = 0;
				gs.restart_id = (g < E.n_games / 2) ? -1 : 0;
				gs.match_score[0] = gs.match_score[1] = gs.match_score[2] = gs.match_score[3] = 0;
			}
		}
		else if (sh_id < E.n_openings)
			begin_game(E, g, sh_id, tid, scratch);
		else if (tid == 0)
		{
			gs.active = 0;
			gs.restart_id = -1; // waits for an opening like a finished game
		}
	}

	/* ADV_THREADS threads per game that must move: the compaction of a large tree (2000 nodes, 250 k edges: 6 MB) is a chain of dependent
	 * load -> store rounds per wave, so its duration falls with the number of waves that copy (256 -> 1024 threads: k_advance 0.36 -> see
	 * DESIGN 6.1); the other games' workgroups leave at once. */
	template<bool MERGED> // (MERGED: as k_search_spec's)
	__global__ __launch_bounds__(ADV_THREADS) void k_advance(EngineDev E)
	{
		constexpr int TPB = ADV_THREADS, WAVES = ADV_THREADS / 64;
		__shared__ u64 scratch[WAVES];
		__shared__ float red_v[WAVES];
		__shared__ int red_i[WAVES];
		__shared__ int sh_int[8];
		__shared__ int scan_nodes[TPB], scan_edges[TPB];
		__shared__ uint16_t cell_edge[MAXHW], entry_cell[MAXHW]; // format-201 sample: edge of a cell (+1, bit 15 = visited or proven), cells with an entry
		__shared__ uint32_t sh_max[3];
		const int g = E.g0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
		GameState &gs = E.games[g];
		if (!gs.active || gs.error != 0 || !gs.need_move || gs.solve_pending || gs.grow_pending)
			return;
		use_game_arenas(E, g);
		if constexpr (MERGED)
			use_player_search(E, g); // (the final selector is the moving player's; its partner's tree is only rebased)
		DNode *nodes = nodes_of(E, g, gs.arena);
		DEdge *edges = edges_of(E, g, gs.arena);
		const int n = E.n;
		if (E.shared_tree && E.search_buffers > 1)
		{ // Search::cleanup (Search.cpp:233-242) of every thread before the move: the OTHER buffer's leaves — selected, solved, in the
		  // network or back from it — are dropped and their virtual losses taken back (SearchThread.cpp:108-109 after asynchronous_run's break)
			if (wave == 0)
				for (int r = 0; r < E.n_games; r++)
				{
					if (r >= E.grp_first && r < E.grp_first + E.grp_count)
						continue; // this buffer was expanded and backed up by k_expand just before
					GameState &os = E.games[r];
					const int pending = os.n_tasks;
					for (int k = 0; k < pending; k++)
					{
						const DTask &t = E.tasks[static_cast<size_t>(r) * E.batch + k];
						cancel_virtual_loss(nodes, edges, t, t.path_len, lane);
						wave_sync();
					}
					if (lane == 0)
						os.n_tasks = 0;
				}
			__threadfence_block();
			__syncthreads();
		}
		const DNode root = nodes[gs.root];

		// ---- final selector: "best" (EdgeSelector.cpp:515-536) or max_visit / min_visit / max_value / max_policy (:476-514) ----
		float best_value = -3.402823466e+38f;
		int best = 0x7FFFFFFF;
		for (int i = tid; i < root.n_edges; i += TPB)
		{
			const DEdge e = edges[root.edge_begin + i];
			float value;
			switch (E.final_selector)
			{
				default:
					switch (s_pv(e.score))
					{
						case 0:
							value = -1.0e8f + s_distance(e.score);
							break;
						case 3:
							value = +1.0e8f - s_distance(e.score);
							break;
						default:
							value = e.visits + (e.win + 0.5f * e.draw) * root.visits + 0.001f * e.prior;
							break;
					}
					break;
				case 1:
					value = e.visits;
					break;
				case 2:
					value = -e.visits;
					break;
				case 3:
					switch (s_pv(e.score))
					{
						case 0:
							value = -1000.0f + s_distance(e.score);
							break;
						case 1:
							value = 0.5f; // Value::draw().getExpectation()
							break;
						case 3:
							value = +1000.0f - s_distance(e.score);
							break;
						default:
							value = e.win + 0.5f * e.draw;
							break;
					}
					break;
				case 4:
					value = e.prior;
					break;
				case 5:
				{ // LCB (EdgeSelector.cpp:446-475): lower confidence bound on unproven edges, proven ones by distance
					const int pv = s_pv(e.score);
					if (pv == 0)
						value = -1.0e6f + s_distance(e.score) + e.prior;
					else if (pv == 3)
						value = +1.0e6f - s_distance(e.score) + e.prior;
					else
					{
						const int vl = e.flag_vl & 0x7FFF;
						const float visits = 1.0e-8f + e.visits;
						const float vl_factor = visits / (visits + static_cast<float>(vl));
						const float Q = (e.visits > 0) ? (e.win + 0.5f * e.draw) : (root.win + 0.5f * root.draw);
						const float parent_log_visit = static_cast<float>(det_log(static_cast<double>(root.visits + root.vl)));
						const float U = E.c_puct * sqrtf(parent_log_visit / (1.0f + e.visits + vl));
						value = Q * vl_factor - U;
					}
					break;
				}
			}
			if (value > best_value)
			{
				best_value = value;
				best = i;
			}
		}
		wave_argmax(best_value, best);
		if (lane == 0)
		{
			red_v[wave] = best_value;
			red_i[wave] = best;
		}
		__syncthreads();
		if (tid == 0)
		{
			for (int w = 1; w < WAVES; w++)
				if (red_v[w] > red_v[0] || (red_v[w] == red_v[0] && red_i[w] < red_i[0]))
				{
					red_v[0] = red_v[w];
					red_i[0] = red_i[w];
				}
			sh_int[4] = red_i[0];
		}
		__syncthreads();
		const int best_edge = sh_int[4];
		const uint32_t mv = edges[root.edge_begin + best_edge].move;

		// ---- the sample in dataset format 201 (SearchDataPack of the root -> SearchDataStorage_v201::loadFrom + serialize,
		//      dataset/data_packs.cpp:24-43, dataset/SearchDataStorage.cpp:326-374,410-419), quantised here so that 6 bytes per visited
		//      cell leave the device instead of 24 per root edge ----
		int n_entries = 0;
		if (E.record_format & 2)
		{
			for (int i = tid; i < E.hw; i += TPB)
				cell_edge[i] = 0;
			if (tid < 3)
				sh_max[tid] = 0u;
			__syncthreads();
			for (int i = tid; i < root.n_edges; i += TPB)
			{ // scatter the edges over the board; the maxima that become the three scales (non-negative floats order like their bits)
				const DEdge e = edges[root.edge_begin + i];
				const int cell = ((e.move >> 2) & 127) * n + ((e.move >> 9) & 127);
				const bool natural = e.visits > 0 || s_proven(e.score);
				cell_edge[cell] = static_cast<uint16_t>((i + 1) | (natural ? 0x8000 : 0));
				const float wd = fmaxf(e.win, e.draw);
				atomicMax(&sh_max[0], __float_as_uint((e.prior > 0.0f) ? e.prior : 0.0f));
				atomicMax(&sh_max[1], __float_as_uint((wd > 0.0f) ? wd : 0.0f));
				atomicMax(&sh_max[2], static_cast<uint32_t>(max(e.visits, 0)));
			}
			__syncthreads();
			// which cells get an entry: visited or proven ones, and any cell 255 or more past the previous entry (:333-337, in cell order)
			if (E.hw <= 255)
			{ // no cell can be 255 past anything: the entries are the flagged cells, compacted in order by the first wave
				if (wave == 0)
				{
					int count = 0;
					for (int base = 0; base < E.hw; base += 64)
					{
						const int i = base + lane;
						const bool flagged = (i < E.hw) && (cell_edge[i] & 0x8000);
						const u64 m = __ballot(flagged);
						if (flagged)
							entry_cell[count + __popcll(m & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))))] = static_cast<uint16_t>(i);
						count += __popcll(m);
					}
					if (lane == 0)
						sh_int[5] = count;
				}
			}
			else if (tid == 0)
			{
				int last = 0, count = 0;
				for (int i = 0; i < E.hw; i++)
					if ((cell_edge[i] & 0x8000) || (i - last) >= 255)
					{
						entry_cell[count++] = static_cast<uint16_t>(i);
						last = i;
					}
				sh_int[5] = count;
			}
			__syncthreads();
			n_entries = sh_int[5];
		}
		if (tid == 0)
		{
			// ---- sample record (GameGenerator.cpp:166-171): the header is written whenever its slot exists, so that the host never
			//      reads a slot that was reserved but not filled; a part that does not fit is left out and stops the game with ERR_RECORDS ----
			const int rec = atomicAdd(&E.counters[3], 1);
			int eoff = -1, soff = -1;
			const int sbytes = v201::HEADER_BYTES + v201::ENTRY_BYTES * n_entries;
			bool fits = rec < E.record_cap;
			if (E.record_format & 1)
			{
				eoff = atomicAdd(&E.counters[4], static_cast<int>(root.n_edges));
				if (eoff + root.n_edges > E.record_edge_cap)
				{
					eoff = -1;
					fits = false;
				}
			}
			if (E.record_format & 2)
			{
				soff = atomicAdd(&E.counters[6], (sbytes + 3) & ~3);
				if (soff + sbytes > E.sample_cap)
				{
					soff = -1;
					fits = false;
				}
			}
			sh_int[0] = (rec < E.record_cap) ? rec : -1;
			sh_int[1] = eoff;
			sh_int[6] = soff;
			sh_int[7] = fits ? 1 : 0;
		}
		__syncthreads();
		const int rec = sh_int[0], eoff = sh_int[1], soff = sh_int[6];
		if (eoff >= 0)
			for (int i = tid; i < root.n_edges; i += TPB)
				E.record_edges[eoff + i] = edges[root.edge_begin + i];
		if (soff >= 0)
		{
			const float prior_scale = v201::prior_scale(__uint_as_float(sh_max[0])), value_scale = v201::value_scale(__uint_as_float(sh_max[1]));
			const float visit_scale = v201::visit_scale(fmaxf(1.0f, static_cast<float>(sh_max[2])));
			uint8_t *out = E.samples + soff;
			if (tid == 0)
			{
				uint16_t *h16 = reinterpret_cast<uint16_t*>(out);
				h16[0] = static_cast<uint16_t>(v201::ScaleFormat::encode(value_scale));
				h16[1] = static_cast<uint16_t>(v201::ScaleFormat::encode(prior_scale));
				h16[2] = static_cast<uint16_t>(v201::ScaleFormat::encode(visit_scale));
				h16[3] = root.score;
				h16[4] = static_cast<uint16_t>(gs.n_moves); // stones on the board the root stands for
				h16[5] = static_cast<uint16_t>((root.flags >> 3) & 7);
				*reinterpret_cast<uint32_t*>(out + 12) = static_cast<uint32_t>(n_entries);
			}
			for (int k = tid; k < n_entries; k += TPB)
			{
				const int cell = entry_cell[k], previous = (k > 0) ? entry_cell[k - 1] : 0;
				const int ei = (cell_edge[cell] & 0x7FFF) - 1;
				int visits = 0;
				float prior = 0.0f, win = 0.0f, draw = 0.0f;
				uint32_t score = s_unknown(0); // a filler cell without an edge: the SearchDataPack defaults (Score(), Value())
				if (ei >= 0)
				{
					const DEdge e = edges[root.edge_begin + ei];
					visits = e.visits;
					prior = e.prior;
					win = e.win;
					draw = e.draw;
					score = e.score;
				}
				uint8_t *q = out + v201::HEADER_BYTES + v201::ENTRY_BYTES * k;
				q[0] = static_cast<uint8_t>(cell - previous);
				q[1] = static_cast<uint8_t>(v201::VisitFormat::encode(static_cast<float>(visits) / visit_scale));
				q[2] = static_cast<uint8_t>(v201::PriorFormat::encode(prior / prior_scale));
				q[3] = static_cast<uint8_t>(v201::score_code(score));
				q[4] = static_cast<uint8_t>(v201::PriorFormat::encode(win / value_scale));
				q[5] = static_cast<uint8_t>(v201::PriorFormat::encode(draw / value_scale));
			}
		}
		if (tid == 0 && !sh_int[7])
			gs.error = ERR_RECORDS;

		// ---- Game::makeMove + getOutcome (Game.cpp:104-122, rules.cpp:110-133) ----
		const int s = mv & 3, r = (mv >> 2) & 127, c = (mv >> 9) & 127, cell = r * n + c;
		if (tid == 0)
		{
			gs.board[cell] = static_cast<uint8_t>(s);
			gs.cboard[cell >> 5] |= static_cast<u64>(s) << (2 * (cell & 31));
			gs.moves[gs.n_moves] = static_cast<uint16_t>(mv);
			gs.n_moves++;
			gs.sign_to_move = 3 - s;
			gs.need_move = 0;
			gs.noise_ready = 0; // prepare_search creates a fresh selector for the next move (GameGenerator.cpp:181-183)
			gs.stats[8]++;
			atomicAdd(&E.counters[5], 1);
			bool win = false;
			for (int d = 0; d < 4; d++)
			{
				uint32_t pattern = 0;
				for (int k = -5, shf = 0; k <= 5; k++, shf += 2)
				{
					const int rr = r + k * row_step(d), cc = c + k * col_step(d);
					uint32_t v = (rr >= 0 && rr < n && cc >= 0 && cc < n) ? gs.board[rr * n + cc] : 3u;
					if (k == 0)
						v = 0;
					pattern |= v << shf;
				}
				const uint8_t e = E.t_pattern[narrow(pattern)];
				if (((s == 1) ? (e & 15) : (e >> 4)) == 6)
					win = true;
			}
			int outcome = 0;
			if (win)
				outcome = (s == 1) ? 2 : 3;
			else if (E.rules == AGX_RENJU && s == 1 && renju_static_foul(E.t_pattern, E.t_threat, gs.board, n, cell))
				outcome = 3; // a foul of the cross player loses the game (rules.cpp:127-128)
			else if (gs.n_moves >= E.draw_after)
				outcome = 1;
			gs.outcome = outcome;
			sh_int[2] = outcome;
			sh_int[3] = -1;
			if (rec >= 0)
			{
				MoveRecordHeader h;
				h.game_serial = gs.opening_id;
				h.move_number = gs.n_moves - 1;
				h.move = static_cast<uint16_t>(mv);
				h.root_score = root.score;
				h.root_visits = root.visits;
				h.root_win = root.win;
				h.root_draw = root.draw;
				h.n_edges = (eoff >= 0) ? root.n_edges : 0;
				h.edge_offset = eoff;
				h.root_flags = (root.flags >> 3) & 7; // DNode flags 8 / 16 / 32
				h.game_slot = g;
				h.game_index = gs.games_done;
				h.sample_offset = soff;
				h.sample_bytes = (soff >= 0) ? v201::HEADER_BYTES + v201::ENTRY_BYTES * n_entries : 0;
				h.outcome = outcome;
				E.records[rec] = h;
			}
			if (outcome != 0)
			{ // game over (GameGenerator.cpp:104-114 -> GAME_NOT_STARTED): k_assign_openings / k_restart give the slot its next opening
				const int ge = atomicAdd(&E.counters[7], 1);
				if (ge < E.game_end_cap)
				{ // setOutcome + addMoves(game.getMoves()) (:107-108)
					GameEndRecord &r = E.game_ends[ge];
					r.game_serial = gs.opening_id;
					r.game_slot = g;
					r.game_index = gs.games_done;
					r.outcome = outcome;
					r.n_moves = gs.n_moves;
					for (int i = 0; i < gs.n_moves; i++)
						r.moves[i] = gs.moves[i];
				}
				else
					gs.error = ERR_RECORDS;
				gs.games_done++;
				atomicAdd(&E.counters[2], 1);
				gs.active = 0;
				gs.restart_id = -1;
			}
		}
		__syncthreads();
		if (E.match_mode)
		{ // EvaluationGame.cpp:126-143: the move goes into the shared game, the OTHER player gets setBoard; this tree is left as it
		  // is until its player's next turn (two plies on)
			const int p = (g + E.n_games / 2) % E.n_games;
			GameState &ps = E.games[p];
			for (int i = tid; i < E.hw; i += TPB)
				ps.board[i] = gs.board[i];
			if (tid < BWORDS)
				ps.cboard[tid] = gs.cboard[tid];
			if (tid == 0)
			{
				ps.moves[gs.n_moves - 1] = static_cast<uint16_t>(mv);
				ps.n_moves = gs.n_moves;
				ps.sign_to_move = gs.sign_to_move;
				ps.outcome = sh_int[2];
				gs.active = 0;
				if (sh_int[2] != 0)
				{ // both trees wait; the first player's tree carries the restart request of the pair
					ps.games_done++;
					GameState &lead = E.games[min(g, p)];
					GameState &part = E.games[max(g, p)];
					part.restart_id = 0;
					// a match is two games on one opening with the colours swapped (EvaluationGame.cpp:44-71): after the first game the
					// pair starts again from the same opening, after the second it waits for a new one
					lead.restart_id = (lead.games_done % 2 == 1) ? lead.opening_id + 1 : -1;
					const int first_won = (sh_int[2] == 2 && lead.my_sign == 1) || (sh_int[2] == 3 && lead.my_sign == 2);
					lead.match_score[(sh_int[2] == 1) ? 1 : (first_won ? 0 : 2)]++;
				}
				else
				{
					ps.active = 1;
					ps.need_move = 0;
					ps.noise_ready = 0;
				}
			}
			__syncthreads();
			if (sh_int[2] == 0)
				rebase_tree<TPB>(E, p, tid, scratch, scan_nodes, scan_edges);
			return;
		}
		if (E.shared_tree)
		{ // every SearchThread's Search sees the move: Search::setBoard -> AlphaBetaSearch::increaseGeneration; a finished game stops them all
		  // (no prepare_search behind the move that ends a game: the generation stays, as record 0's does — begin_game raises them all alike,
		  // so that a thread's solver sees one generation in the tree's next game, whichever of its task buffers a leaf sits in)
			for (int t = 1 + tid; t < E.n_games; t += TPB)
			{
				GameState &ls = E.games[t];
				if (sh_int[2] == 0)
					ls.generation = (ls.generation + 1) % 64;
				ls.outcome = sh_int[2];
				ls.n_moves = gs.n_moves;
				if (sh_int[2] != 0)
					ls.active = 0;
			}
		}
		if (sh_int[2] != 0)
			return;
		rebase_tree<TPB>(E, g, tid, scratch, scan_nodes, scan_edges);
	}

	/*
	 * Finished games take the next openings of the pool in GAME ORDER (not in the order their workgroups happen to finish), so a
	 * run is reproducible: one workgroup scans the games of the launch's range, numbers the waiting ones and reserves that many
	 * openings; games for which none is left keep waiting (agx_engine_add_openings can supply more).
	 */
	/* A finished game takes its next opening.  In the reference every GameGenerator draws its own openings (OpeningGenerator per generator,
	 * GameGenerator.cpp:46-77); here slot s of S takes openings s, s + S, s + 2 S, ... — a function of the slot and of how many games it has
	 * played, NOT of which slot finished first, so a pool plays the same games however it is sliced into groups and however their launches
	 * interleave on their streams.  A slot whose next opening is not in the list yet waits (agx_engine_add_openings).  counters[1] keeps the
	 * high-water mark (openings_taken). */
	__device__ __forceinline__ void assign_openings(const EngineDev &E, int count)
	{ // (1024 threads of one workgroup)
		const int slots = E.shared_tree ? 1 : (E.match_mode ? E.n_games / 2 : E.n_games);
		for (int i = threadIdx.x; i < count; i += 1024)
		{
			GameState &gs = E.games[E.g0 + i];
			if (gs.restart_id != -1)
				continue;
			// (match mode: a pair plays every opening twice, colours swapped — games_done counts games, the opening changes every other one)
			const int round = E.match_mode ? gs.games_done / 2 : gs.games_done;
			const long long id = static_cast<long long>(E.g0 + i) + static_cast<long long>(slots) * round;
			if (id < E.n_openings)
			{
				gs.restart_id = static_cast<int>(id) + 1;
				atomicMax(&E.counters[1], static_cast<int>(id) + 1);
			}
		}
	}
	__global__ __launch_bounds__(1024) void k_assign_openings(EngineDev E, int count)
	{
		assign_openings(E, count);
	}
	/* the workgroup that finishes a game's LAST part (of k_arena_copy, k_clear_tables) does what used to be the launch behind it: every part
	 * makes its writes visible (agent-scope fence), takes a ticket, and the holder of the last ticket knows that all the others are through */
	__device__ __forceinline__ bool last_part_of(int *counter, int parts)
	{
		__shared__ int sh_last;
		__threadfence();
		__syncthreads();
		if (threadIdx.x == 0)
		{
			const int ticket = __hip_atomic_fetch_add(counter, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
			sh_last = (ticket == parts - 1) ? 1 : 0;
			if (sh_last)
				__hip_atomic_store(counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (ready for the game's next time)
		}
		__syncthreads();
		const bool last = sh_last != 0;
		if (last)
			__threadfence();
		return last;
	}
	/*
	 * Tree::clear + AlphaBetaSearch::clear for the games about to restart, spread over `parts` workgroups per game: a 4 Mi-entry
	 * solver table is 64 MB, which one workgroup takes a millisecond to fill — longer than every other kernel of the step but two.
	 * Match mode: both trees of a pair whose first player's tree carries the restart request; the node tables stay (Player keeps
	 * its tree).
	 */
	__global__ __launch_bounds__(256) void k_clear_tables(EngineDev E, int parts, int restart)
	{ // restart != 0 (self-play pools with a tree per game): the workgroup that finishes a game's last part starts its next game (k_restart's work)
		__shared__ u64 scratch[4];
		const int g = E.g0 + blockIdx.x / parts, part = blockIdx.x % parts, tid = threadIdx.x;
		const int asks = E.shared_tree ? 0 : (E.match_mode ? g % (E.n_games / 2) : g);
		if (E.games[asks].restart_id <= 0)
			return;
		ulonglong2 *tt = reinterpret_cast<ulonglong2*>(E.tt + static_cast<size_t>(g % E.tt_mod) * (E.tt_bucket_mask + 1ull) * 8ull);
		const size_t entries = (E.tt_bucket_mask + 1ull) * 4ull;
		const size_t per = (entries + parts - 1) / parts;
		const size_t end = (per * (part + 1) < entries) ? per * (part + 1) : entries;
		ulonglong2 empty;
		empty.x = 0ull;
		empty.y = tt_pack(0, 0, s_unknown(0), 0);
		for (size_t i = per * part + tid; i < end; i += 256)
			tt[i] = empty;
		if (!E.match_mode)
		{
			int *ht = ht_of(E, g);
			for (int i = part * 256 + tid; i < E.games[g].ht_cap; i += parts * 256)
				ht[i] = 0;
		}
		if (restart != 0 && last_part_of(E.parts_done + E.n_games + g, parts))
			begin_game(E, g, E.games[g].restart_id - 1, tid, scratch, true); // (every table of the game is empty and visible: last_part_of)
	}
	__global__ __launch_bounds__(256) void k_restart(EngineDev E)
	{
		__shared__ u64 scratch[4];
		const int g = E.g0 + blockIdx.x, tid = threadIdx.x;
		const int id = E.games[E.shared_tree ? 0 : g].restart_id; // (tournament search: thread 0's request counts for every search thread,
		if (id <= 0)                                              //  and thread 0 is restarted by a later launch than the others)
			return;
		__syncthreads();
		begin_game(E, g, id - 1, tid, scratch, true); // k_clear_tables ran just before
	}

	/*
	 * Match mode: one workgroup per pair.  EvaluationGame.cpp:77-106: both solvers are cleared, the opening is loaded into the
	 * shared game, the first player takes cross in the first game of a match and circle in the second, and only the player to
	 * move gets setBoard — on a tree that still holds its previous game (Player keeps its Tree; what the new position cannot reach
	 * is dropped by the cleanup inside setBoard).
	 */
	__global__ __launch_bounds__(256) void k_match_restart(EngineDev E)
	{
		__shared__ u64 scratch[4];
		__shared__ int scan_nodes[256], scan_edges[256];
		const int lead = blockIdx.x, part = lead + E.n_games / 2, tid = threadIdx.x;
		const int id = E.games[lead].restart_id - 1;
		if (id < 0)
			return;
		__syncthreads();
		const uint16_t *op = E.openings + static_cast<size_t>(id) * OPENING_CAP;
		const int count = op[0];
		for (int k = 0; k < 2; k++)
		{
			const int t = k ? part : lead;
			GameState &gs = E.games[t]; // (both solver tables were emptied by k_clear_tables just before)
			for (int i = tid; i < E.hw; i += 256)
				gs.board[i] = 0;
			if (tid < BWORDS)
				gs.cboard[tid] = 0;
			__syncthreads();
			if (tid == 0)
			{
				int sign = 1;
				for (int i = 0; i < count; i++)
				{
					const uint32_t mv = op[1 + i];
					const int cell = ((mv >> 2) & 127) * E.n + ((mv >> 9) & 127);
					gs.board[cell] = static_cast<uint8_t>(mv & 3);
					gs.cboard[cell >> 5] |= static_cast<u64>(mv & 3) << (2 * (cell & 31));
					gs.moves[i] = static_cast<uint16_t>(mv);
					sign = 3 - static_cast<int>(mv & 3);
				}
				gs.sign_to_move = sign;
				gs.n_moves = count;
				gs.outcome = 0;
				gs.n_tasks = 0;
				gs.need_move = 0;
				gs.solve_pos = 0;
				gs.solve_pending = 0;
				park_forget_game(E, t);
				gs.nn_queued = 0;
				gs.restart_id = 0;
				gs.noise_ready = 0;
				gs.opening_id = id;
				gs.active = 0;
				const int lead_sign = (E.games[lead].games_done % 2 == 0) ? 1 : 2;
				gs.my_sign = k ? 3 - lead_sign : lead_sign;
			}
			__syncthreads();
		}
		const int mover = (E.games[lead].sign_to_move == E.games[lead].my_sign) ? lead : part;
		rebase_tree<256>(E, mover, tid, scratch, scan_nodes, scan_edges);
		if (tid == 0)
			E.games[mover].active = 1;
	}

	/*
	 * Arena heap service, once per step after k_advance: ONE workgroup; its thread 0 is the only allocator, so the per-class free lists
	 * need no lock.  (1) games that ended with a grown bundle give it back and return to class 0 (self-play only: a match player keeps its
	 * tree); (2) games whose expand asked for room get a bundle of the next class reserved (copied over by k_arena_copy).
	 */
	/* The heap and its free lists are shared by the whole pool, and slices of a pool may be stepped on different streams: every access goes
	 * through agent-scope atomics under one spin lock (taken by a single thread of a workgroup, for a handful of words). */
	template<typename T>
	__device__ __forceinline__ T heap_load(T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
	template<typename T>
	__device__ __forceinline__ void heap_store(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
	__device__ void heap_lock(ArenaHeap *h)
	{
		int expected = 0;
		while (!__hip_atomic_compare_exchange_strong(&h->lock, &expected, 1, __ATOMIC_ACQUIRE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
		{
			expected = 0;
			__builtin_amdgcn_s_sleep(2);
		}
	}
	__device__ void heap_unlock(ArenaHeap *h) { __hip_atomic_store(&h->lock, 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT); }
	__device__ void bundle_store(ArenaBundle *dst, const ArenaBundle &b)
	{
		heap_store(&dst->node_off[0], b.node_off[0]);
		heap_store(&dst->node_off[1], b.node_off[1]);
		heap_store(&dst->edge_off[0], b.edge_off[0]);
		heap_store(&dst->edge_off[1], b.edge_off[1]);
		heap_store(&dst->ht_off, b.ht_off);
	}
	__device__ bool arena_alloc(const EngineDev &E, int cls, ArenaBundle &out)
	{ // one calling thread per workgroup
		ArenaHeap *h = E.heap;
		bool ok = true;
		heap_lock(h);
		const int free_count = heap_load(&h->free_count[cls]);
		if (free_count > 0)
		{
			ArenaBundle *src = E.free_bundles + static_cast<size_t>(cls) * h->free_capacity + (free_count - 1);
			out.node_off[0] = heap_load(&src->node_off[0]);
			out.node_off[1] = heap_load(&src->node_off[1]);
			out.edge_off[0] = heap_load(&src->edge_off[0]);
			out.edge_off[1] = heap_load(&src->edge_off[1]);
			out.ht_off = heap_load(&src->ht_off);
			heap_store(&h->free_count[cls], free_count - 1);
		}
		else
		{
			const u64 nodes = static_cast<u64>(E.node_cap) << cls, edges = static_cast<u64>(E.edge_cap) << cls, ht = static_cast<u64>(E.ht_cap) << cls;
			const u64 nc = heap_load(&h->node_cursor), ec = heap_load(&h->edge_cursor), hc = heap_load(&h->ht_cursor);
			if (nc + 2 * nodes > h->node_total || ec + 2 * edges > h->edge_total || hc + ht > h->ht_total)
				ok = false;
			else
			{
				out.node_off[0] = nc;
				out.node_off[1] = nc + nodes;
				out.edge_off[0] = ec;
				out.edge_off[1] = ec + edges;
				out.ht_off = hc;
				heap_store(&h->node_cursor, nc + 2 * nodes);
				heap_store(&h->edge_cursor, ec + 2 * edges);
				heap_store(&h->ht_cursor, hc + ht);
			}
		}
		heap_unlock(h);
		return ok;
	}
	__device__ void arena_free(const EngineDev &E, int cls, const GameState &gs)
	{ // one calling thread per workgroup
		ArenaHeap *h = E.heap;
		ArenaBundle b;
		b.node_off[0] = gs.node_off[0];
		b.node_off[1] = gs.node_off[1];
		b.edge_off[0] = gs.edge_off[0];
		b.edge_off[1] = gs.edge_off[1];
		b.ht_off = gs.ht_off;
		heap_lock(h);
		const int free_count = heap_load(&h->free_count[cls]);
		if (free_count < h->free_capacity)
		{ // (the lists hold one entry per game and class: always true; a bundle that found no room would be leaked, never handed out twice)
			bundle_store(E.free_bundles + static_cast<size_t>(cls) * h->free_capacity + free_count, b);
			heap_store(&h->free_count[cls], free_count + 1);
		}
		heap_unlock(h);
	}
	__global__ __launch_bounds__(1024) void k_arena_service(EngineDev E, int count, int assign_count)
	{ // assign_count > 0: the finished games of the first assign_count take their next openings here as well (k_assign_openings' work, one launch less per cycle)
		__shared__ int sh_list[1024];
		__shared__ int sh_n;
		const int tid = threadIdx.x;
		for (int start = 0; start < count; start += 1024)
		{
			if (tid == 0)
				sh_n = 0;
			__syncthreads();
			const int i = start + tid;
			if (i < count)
			{
				const GameState &gs = E.games[E.g0 + i];
				const bool release = !E.match_mode && gs.restart_id == -1 && gs.arena_class > 0 && gs.grow_pending == 0;
				if (gs.grow_pending == 1 || release)
					sh_list[atomicAdd(&sh_n, 1)] = i;
			}
			__syncthreads();
			if (tid == 0)
			{
				// requests in game order (the lanes appended them in any order): results do not depend on it, the heap layout stays reproducible
				for (int a = 1; a < sh_n; a++)
					for (int b = a; b > 0 && sh_list[b - 1] > sh_list[b]; b--)
					{
						const int tmp = sh_list[b];
						sh_list[b] = sh_list[b - 1];
						sh_list[b - 1] = tmp;
					}
				for (int k = 0; k < sh_n; k++)
				{
					GameState &gs = E.games[E.g0 + sh_list[k]];
					if (gs.grow_pending == 1)
					{
						ArenaBundle nb;
						if (arena_alloc(E, gs.arena_class + 1, nb))
						{
							gs.new_node_off[0] = nb.node_off[0];
							gs.new_node_off[1] = nb.node_off[1];
							gs.new_edge_off[0] = nb.edge_off[0];
							gs.new_edge_off[1] = nb.edge_off[1];
							gs.new_ht_off = nb.ht_off;
							gs.grow_pending = 3;
							atomicAdd(&E.heap->grows, 1);
						}
						else
						{ // heap exhausted: the game carries on in its arenas; if the batch really overflows them, k_expand reports it
							gs.grow_pending = 4;
							atomicAdd(&E.heap->failures, 1);
						}
					}
					else
					{ // a finished game hands its grown bundle back and waits for its next opening in class-0 arenas
						ArenaBundle nb;
						if (arena_alloc(E, 0, nb))
						{
							arena_free(E, gs.arena_class, gs);
							gs.node_off[0] = nb.node_off[0];
							gs.node_off[1] = nb.node_off[1];
							gs.edge_off[0] = nb.edge_off[0];
							gs.edge_off[1] = nb.edge_off[1];
							gs.ht_off = nb.ht_off;
							gs.arena_class = 0;
							gs.node_cap = E.node_cap;
							gs.edge_cap = E.edge_cap;
							gs.ht_cap = E.ht_cap;
							atomicAdd(&E.heap->releases, 1);
						}
					}
				}
			}
			__syncthreads();
		}
		if (assign_count > 0)
			assign_openings(E, assign_count); // (behind the releases: a finished game gives its grown bundle back before it is handed its next opening)
	}
	/* moves a game's tree into the bundle k_arena_service reserved for it: nodes and edges of the active arena copied as they are (indices
	 * stay valid), the node-cache table rebuilt at its new size.  `parts` workgroups per game: the edges (a few MB for a large tree) are
	 * split among parts 1.., part 0 moves the nodes and rebuilds the table; the workgroup that finishes the game's last part switches the game over (arena_commit). */
	/* the old bundle goes onto the free list, the game continues in the new one (ONE acting thread: the heap lock must never be contended by lanes of one wave) */
	__device__ void arena_commit(const EngineDev &E, GameState &gs);
	__global__ __launch_bounds__(256) void k_arena_copy(EngineDev E, int parts)
	{
		const int g = E.g0 + blockIdx.x / parts, part = blockIdx.x % parts, tid = threadIdx.x;
		GameState &gs = E.games[g];
		if (gs.grow_pending != 3)
			return;
		if (part != 0)
		{ // 24-byte edge records copied as 16-byte words (arena regions start at multiples of the even class-0 capacity: 16-byte aligned)
			const uint4 *src_edges = reinterpret_cast<const uint4*>(edges_of(E, g, gs.arena));
			uint4 *dst_edges = reinterpret_cast<uint4*>(E.edges + gs.new_edge_off[gs.arena]);
			const size_t halves = 3 * static_cast<size_t>(gs.n_edges), words = halves / 2;
			for (size_t i = static_cast<size_t>(part - 1) * 256 + tid; i < words; i += static_cast<size_t>(parts - 1) * 256)
				dst_edges[i] = src_edges[i];
			if ((halves & 1) != 0 && part == 1 && tid == 0)
				reinterpret_cast<u64*>(dst_edges)[halves - 1] = reinterpret_cast<const u64*>(src_edges)[halves - 1];
		}
		else
		{
			const int new_ht_cap = E.ht_cap << (gs.arena_class + 1);
			const DNode *src_nodes = nodes_of(E, g, gs.arena);
			DNode *dst_nodes = E.nodes + gs.new_node_off[gs.arena];
			int *ht = E.ht + gs.new_ht_off;
			for (int i = tid; i < new_ht_cap; i += 256)
				ht[i] = 0;
			__syncthreads();
			const int mask = new_ht_cap - 1;
			for (int i = tid; i < gs.n_nodes; i += 256)
			{
				const DNode nd = src_nodes[i];
				dst_nodes[i] = nd;
				int slot = static_cast<int>(nd.hash & static_cast<u64>(mask));
				while (atomicCAS(&ht[slot], 0, i + 1) != 0)
					slot = (slot + 1) & mask;
			}
		}
		// (once a launch of its own, k_arena_commit: the game is switched over by whichever workgroup finishes its last part — the others only READ the game's state,
		//  and none of them is still running when it changes)
		if (last_part_of(E.parts_done + g, parts) && tid == 0)
			arena_commit(E, gs);
	}
	__device__ void arena_commit(const EngineDev &E, GameState &gs)
	{
		const int cls = gs.arena_class + 1;
		arena_free(E, gs.arena_class, gs);
		gs.node_off[0] = gs.new_node_off[0];
		gs.node_off[1] = gs.new_node_off[1];
		gs.edge_off[0] = gs.new_edge_off[0];
		gs.edge_off[1] = gs.new_edge_off[1];
		gs.ht_off = gs.new_ht_off;
		gs.arena_class = cls;
		gs.node_cap = E.node_cap << cls;
		gs.edge_cap = E.edge_cap << cls;
		gs.ht_cap = E.ht_cap << cls;
		gs.grow_count++;
		gs.grow_pending = 2;
	}

	/* Tree::setBoard(board, signToMove) + Search::setBoard + Search::cleanup for ONE game driven from outside (evaluation/Player.cpp:100-110):
	 * the position becomes the tree's base board, every cached state that can still be reached from it is kept (NodeCache::cleanup:
	 * compaction into the other arena, table rebuilt), the root is whatever the cache holds for it, abandoned tasks are dropped and the
	 * solver table ages by one generation (Tree.cpp:128-151, Search.cpp:112-115,233-242). */
	/* Search::cleanup (Search.cpp:233-242) from outside: the leaves selected but not expanded — of every task buffer that works on the tree —
	 * are dropped and their virtual losses taken back (Tree::cancelVirtualLoss, Tree.cpp:377-384).  One wave per tree. */
	__global__ __launch_bounds__(64) void k_cancel_pending(EngineDev E)
	{
		const int tg = E.shared_tree ? 0 : E.g0 + blockIdx.x, lane = threadIdx.x;
		GameState &gs = E.games[tg];
		use_game_arenas(E, tg);
		DNode *nodes = nodes_of(E, tg, gs.arena);
		DEdge *edges = edges_of(E, tg, gs.arena);
		const int first = E.shared_tree ? 0 : tg, last = E.shared_tree ? E.n_games - 1 : tg;
		for (int r = first; r <= last; r++)
		{
			GameState &os = E.games[r];
			const int pending = os.n_tasks;
			for (int k = 0; k < pending; k++)
			{
				const DTask &t = E.tasks[static_cast<size_t>(r) * E.batch + k];
				cancel_virtual_loss(nodes, edges, t, t.path_len, lane);
				wave_sync();
			}
			if (lane == 0)
			{
				os.n_tasks = 0;
				os.solve_pos = 0;
				os.solve_pending = 0;
				park_forget_game(E, r);
			}
		}
	}
	__global__ __launch_bounds__(256) void k_set_board(EngineDev E, int g, const uint8_t *board, int sign_to_move, int force_remove_root)
	{
		__shared__ u64 scratch[4];
		__shared__ int scan_nodes[256], scan_edges[256];
		const int tid = threadIdx.x;
		GameState &gs = E.games[g];
		for (int i = tid; i < E.hw; i += 256)
			gs.board[i] = board[i];
		if (tid < BWORDS)
			gs.cboard[tid] = 0;
		__syncthreads();
		if (tid == 0)
		{
			int stones = 0;
			for (int cell = 0; cell < E.hw; cell++)
				if (board[cell] != 0)
				{
					gs.cboard[cell >> 5] |= static_cast<u64>(board[cell] & 3) << (2 * (cell & 31));
					stones++;
				}
			gs.sign_to_move = sign_to_move;
			gs.n_moves = stones;
			gs.outcome = 0;
			gs.n_tasks = 0;
			gs.need_move = 0;
			gs.solve_pos = 0;
			gs.solve_pending = 0;
			park_forget_game(E, g);
			gs.grow_pending = 0;
			gs.noise_ready = 0;
			gs.restart_id = 0;
			gs.active = 1;
		}
		__syncthreads();
		if (force_remove_root)
			rebase_tree<256, true>(E, g, tid, scratch, scan_nodes, scan_edges);
		else
			rebase_tree<256>(E, g, tid, scratch, scan_nodes, scan_edges);
		if (E.shared_tree)
		{ // every task buffer of the tree follows (its solver table ages with the tree's, Search::setBoard -> increaseGeneration)
			__syncthreads();
			for (int t = 1 + tid; t < E.n_games; t += 256)
			{
				GameState &ls = E.games[t];
				ls.generation = (ls.generation + 1) % 64;
				ls.outcome = 0;
				ls.n_moves = gs.n_moves;
				ls.n_tasks = 0;
				ls.active = 1;
			}
		}
	}

	/* GameGenerator::load (GameGenerator.cpp:131-141) for pool slot g: the saved game (its moves so far) with an EMPTY tree and solver table — the
	 * reference's checkpoint holds the Game and the samples collected so far, the search starts again with prepare_search */
	__global__ __launch_bounds__(256) void k_restore_game(EngineDev E, int g, const uint16_t *moves, int count, int opening_id, int nn_queued)
	{
		__shared__ u64 scratch[4];
		if (threadIdx.x == 0)
			E.games[g].generation = 0; // a loaded GameGenerator owns a new AlphaBetaSearch: its table's generation counts from 0 again (SharedHashTable.hpp:126,
			                           // :155 — prepare_search makes it 1), and the ageing of entries (depth - (generation - entry's), modulo 64) follows that count
		__syncthreads();
		begin_game(E, g, opening_id, threadIdx.x, scratch, false, moves, count);
		if (threadIdx.x == 0)
			E.games[g].nn_queued = nn_queued;
	}

	/* what a search loop asks the tree between two steps (Tree::getSimulationCount / isRootProven / getNodeCount under the tree lock,
	 * SearchThread.cpp:181-199) */
	__global__ void k_root_summary(EngineDev E, int g, int *out)
	{
		const GameState &gs = E.games[g];
		int visits = 0, proven = 0;
		if (gs.root >= 0)
		{
			const DNode &r = nodes_of(E, g, gs.arena)[gs.root];
			visits = r.visits;
			proven = s_proven(r.score) ? 1 : 0;
		}
		out[0] = visits;
		out[1] = proven;
		out[2] = gs.n_nodes;
		out[3] = gs.error;
	}
	/* agx_engine_match_summary: the pairs' match scores and finished games added up by one workgroup (what EvaluationManager sums per player,
	 * evaluation/EvaluationManager.cpp), 32 bytes for a polling loop instead of every pair's GameState.  out[0..2] = games won / drawn / lost
	 * by the first player, out[3] = games finished.  The pairs' records are the first n_games / 2 (the first players' trees). */
	__global__ __launch_bounds__(256) void k_match_summary(EngineDev E, long long *out)
	{
		__shared__ long long part[4][4]; // [wave][sum]
		const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pairs = E.n_games / 2;
		long long sum[4] = { 0, 0, 0, 0 };
		for (int i = tid; i < pairs; i += 256)
		{
			const GameState &gs = E.games[i];
			sum[0] += gs.match_score[0];
			sum[1] += gs.match_score[1];
			sum[2] += gs.match_score[2];
			sum[3] += gs.games_done;
		}
		for (int k = 0; k < 4; k++)
		{
			for (int o = 32; o > 0; o >>= 1)
				sum[k] += __shfl_down(sum[k], o, 64);
			if (lane == 0)
				part[wave][k] = sum[k];
		}
		__syncthreads();
		if (tid < 4)
			out[tid] = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
	}

	/* Behind every k_advance of a match pool that tracks its pairs, ONE workgroup: the pairs in index order, 256 at a time.  A pair whose
	 * games_done is even and above its shadow's has finished an opening: points = 2 dW + dD against the shadow, one entry, hist[points]++,
	 * the shadow follows.  The entries are placed by an ordered compaction (wave ballot, prefix over the four waves in LDS, running base from
	 * chunk to chunk), so the log's order is launch, then pair index, whatever the scheduling.  This kernel is the only writer of everything
	 * it touches and its launches follow each other on the step's stream: plain loads and stores, no atomics.  What cannot be a result — more
	 * than one opening since the shadow, or scores that do not add up to two games — raises a flag and is neither logged nor counted; the
	 * shadow is resynchronised all the same.  A full log still counts the result (head[0..5]), sets flag 1 and writes nothing. */
	__global__ __launch_bounds__(256) void k_match_pair_log(EngineDev E, PairLogDev L)
	{
		__shared__ int wave_found[4];
		__shared__ long long part[4][6]; // [wave][hist 0..4, flags]
		const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, pairs = E.n_games / 2;
		const int launch = static_cast<int>(L.head[7]);
		long long seen = L.head[5]; // = the log position of the next result
		int hist[5] = { 0, 0, 0, 0, 0 }, flags = 0; // (wave-uniform)
		for (int first = 0; first < pairs; first += 256)
		{
			const int i = first + tid;
			bool result = false;
			int points = 0, round = 0, bad = 0;
			if (i < pairs)
			{
				const GameState &gs = E.games[i];
				const int done = gs.games_done;
				const int4 was = L.shadow[i];
				if ((done & 1) == 0 && done > was.x)
				{
					const int won = gs.match_score[0], drawn = gs.match_score[1], lost = gs.match_score[2];
					if (done - was.x > 2)
						bad |= 2;
					if ((won - was.y) + (drawn - was.z) + (lost - was.w) != 2)
						bad |= 4;
					result = (bad == 0);
					points = 2 * (won - was.y) + (drawn - was.z);
					round = done / 2 - 1;
					L.shadow[i] = make_int4(done, won, drawn, lost);
				}
			}
			const u64 found = __ballot(result);
			if (lane == 0)
				wave_found[wave] = __popcll(found);
			for (int k = 0; k < 5; k++)
				hist[k] += __popcll(__ballot(result && points == k));
			flags |= (__ballot((bad & 2) != 0) != 0ull ? 2 : 0) | (__ballot((bad & 4) != 0) != 0ull ? 4 : 0);
			__syncthreads();
			int before = 0, total = 0;
			for (int w = 0; w < 4; w++)
			{
				before += (w < wave) ? wave_found[w] : 0;
				total += wave_found[w];
			}
			if (result)
			{
				const long long pos = seen + before + __popcll(found & ((1ull << lane) - 1ull));
				if (pos < L.capacity)
				{
					AgxPairResult r;
					r.pair = i;
					r.round = round;
					r.points = points;
					r.launch = launch;
					L.entries[pos] = r;
				}
			}
			seen += total;
			__syncthreads(); // (wave_found is rewritten by the next chunk)
		}
		if (lane == 0)
		{
			for (int k = 0; k < 5; k++)
				part[wave][k] = hist[k];
			part[wave][5] = flags;
		}
		__syncthreads(); // (every thread has read head[5] and head[7] by now)
		if (tid < 5)
			L.head[tid] += part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
		else if (tid == 5)
			L.head[5] = seen;
		else if (tid == 6)
			L.head[6] |= part[0][5] | part[1][5] | part[2][5] | part[3][5] | (seen > L.capacity ? 1 : 0);
		else if (tid == 7)
			L.head[7] = launch + 1;
		else if (tid == 8)
			L.head[8] = (seen < L.capacity) ? seen : L.capacity;
	}

	/* Tree::getInfo(moves) / the principal variation (agx_engine_node_info / agx_engine_principal_variation): read-only walks over one tree's
	 * node cache, one wave per walk.  The position is the compressed board in LDS plus the node-cache key, updated per ply like the descent
	 * updates them (k_select); the colours alternate from the base board's side to move (Tree.cpp:403-424). */
	struct QueryWalk
	{
			u64 hash;
			int sign;
			bool valid; // false once a move hit an occupied cell: the reference's empty Node()
	};
	__device__ inline void query_begin(const EngineDev &E, const GameState &gs, u64 *sh_cboard, QueryWalk &q, int lane)
	{
		if (lane < BWORDS)
			sh_cboard[lane] = gs.cboard[lane];
		q.sign = gs.sign_to_move;
		q.hash = full_hash(E, gs.board, q.sign, lane);
		q.valid = true;
		__syncthreads();
	}
	__device__ inline void query_place(const EngineDev &E, u64 *sh_cboard, QueryWalk &q, uint32_t move, int lane)
	{ // (row, col) < n: checked by the host for caller paths, edge moves are cells of the board
		if (!q.valid)
			return;
		const int cell = ((move >> 2) & 127) * E.n + ((move >> 9) & 127), w = cell >> 5, shift = 2 * (cell & 31);
		const bool empty = ((sh_cboard[w] >> shift) & 3ull) == 0;
		__syncthreads();
		if (!empty)
		{
			q.valid = false;
			return;
		}
		if (lane == 0)
			sh_cboard[w] |= static_cast<u64>(q.sign) << shift;
		q.hash ^= E.nc_keys[3 + 3 * cell] ^ E.nc_keys[3 + 3 * cell + q.sign] ^ E.nc_keys[q.sign] ^ E.nc_keys[3 - q.sign];
		q.sign = 3 - q.sign;
		__syncthreads();
	}
	__device__ inline void query_write_node(AgxNodeView *out, const DNode *nd, int lane)
	{ // nd == nullptr: not found
		if (lane != 0)
			return;
		AgxNodeView v;
		v.found = (nd != nullptr) ? 1 : 0;
		v.visits = nd ? nd->visits : 0;
		v.win = nd ? nd->win : 0.0f;
		v.draw = nd ? nd->draw : 0.0f;
		v.moves_left = nd ? nd->moves_left : 0.0f;
		v.score = nd ? nd->score : 0;
		v.flags = nd ? nd->flags : 0;
		v.sign_to_move = nd ? nd->sign_to_move : 0;
		v.depth = nd ? nd->depth : 0;
		v.virtual_loss = nd ? nd->vl : 0;
		v.n_edges = nd ? nd->n_edges : 0;
		*out = v;
	}
	__device__ __forceinline__ void query_write_edge(AgxEdgeView *out, const DEdge &d)
	{
		AgxEdgeView v;
		v.prior = d.prior;
		v.win = d.win;
		v.draw = d.draw;
		v.visits = d.visits;
		v.move = d.move;
		v.score = d.score;
		v.flag_and_virtual_loss = d.flag_vl;
		v.reserved = 0;
		*out = v;
	}
	/* BestEdgeSelector (EdgeSelector.cpp:515-536): the rating of k_advance's default final selector, the same arithmetic */
	__device__ __forceinline__ float best_edge_rating(const DEdge &e, const DNode &parent)
	{
		switch (s_pv(e.score))
		{
			case 0:
				return -1.0e8f + s_distance(e.score);
			case 3:
				return +1.0e8f - s_distance(e.score);
			default:
				return e.visits + (e.win + 0.5f * e.draw) * parent.visits + 0.001f * e.prior;
		}
	}

	/* One wave per path (agx_engine_node_info): path p is moves[offsets[p] .. offsets[p + 1]) */
	__global__ __launch_bounds__(64) void k_node_info(EngineDev E, int t, const uint16_t *moves, const int *offsets, AgxNodeView *out_nodes,
			AgxEdgeView *out_edges, int edges_per_path)
	{
		__shared__ u64 sh_cboard[BWORDS];
		const int p = blockIdx.x, lane = threadIdx.x;
		use_game_arenas(E, t);
		const GameState &gs = E.games[t];
		const DNode *nodes = nodes_of(E, t, gs.arena);
		const DEdge *edges = edges_of(E, t, gs.arena);
		QueryWalk q;
		query_begin(E, gs, sh_cboard, q, lane);
		for (int k = offsets[p]; k < offsets[p + 1] && q.valid; k++)
			query_place(E, sh_cboard, q, moves[k], lane);
		const int found = q.valid ? cache_seek(E, nodes, ht_of(E, t), q.hash, sh_cboard, q.sign, lane) : -1;
		query_write_node(out_nodes + p, (found >= 0) ? nodes + found : nullptr, lane);
		if (found >= 0)
		{
			const DNode &nd = nodes[found];
			const int count = min(static_cast<int>(nd.n_edges), edges_per_path);
			for (int i = lane; i < count; i += 64)
				query_write_edge(out_edges + static_cast<size_t>(p) * edges_per_path + i, edges[nd.edge_begin + i]);
		}
	}

	/* The principal variation (agx_engine_principal_variation, one wave): the path, then BestEdgeSelector's edge and its child while the node
	 * is cached and has edges, at most max_length plies.  out_nodes[k] is the node after k plies (max_length + 1 records). */
	__global__ __launch_bounds__(64) void k_principal_variation(EngineDev E, int t, const uint16_t *moves, int n_moves, int max_length, int *out_length,
			uint16_t *out_pv, AgxEdgeView *out_edges, AgxNodeView *out_nodes)
	{
		__shared__ u64 sh_cboard[BWORDS];
		const int lane = threadIdx.x;
		use_game_arenas(E, t);
		const GameState &gs = E.games[t];
		const DNode *nodes = nodes_of(E, t, gs.arena);
		const DEdge *edges = edges_of(E, t, gs.arena);
		const int *ht = ht_of(E, t);
		QueryWalk q;
		query_begin(E, gs, sh_cboard, q, lane);
		for (int k = 0; k < n_moves && q.valid; k++)
			query_place(E, sh_cboard, q, moves[k], lane);
		int length = 0;
		while (true)
		{
			const int found = q.valid ? cache_seek(E, nodes, ht, q.hash, sh_cboard, q.sign, lane) : -1;
			query_write_node(out_nodes + length, (found >= 0) ? nodes + found : nullptr, lane);
			if (found < 0 || length >= max_length)
				break;
			DNode nd;
			node_head(nd, nodes[found]);
			if (nd.n_edges <= 0)
				break;
			float best_value = -3.402823466e+38f;
			int best = 0x7FFFFFFF;
			for (int i = lane; i < nd.n_edges; i += 64)
			{ // first strict maximum per lane, then the lowest index among the lanes' maxima (k_advance's tie rule)
				const float value = best_edge_rating(edges[nd.edge_begin + i], nd);
				if (value > best_value)
				{
					best_value = value;
					best = i;
				}
			}
			wave_argmax(best_value, best);
			if (best >= nd.n_edges)
				break; // (no edge rated above the floor: only NaN ratings)
			const DEdge chosen = edges[nd.edge_begin + best];
			if (lane == 0)
			{
				out_pv[length] = chosen.move;
				query_write_edge(out_edges + length, chosen);
			}
			query_place(E, sh_cboard, q, chosen.move, lane);
			length++;
		}
		if (lane == 0)
			*out_length = length;
	}
	__global__ void k_reset_counter(int *counter, int *second)
	{
		*counter = 0;
		if (second != nullptr)
			*second = 0;
	}

	/* ------------------------------------------------------------------------------------------------------------ */
	/*
	 * Positions searched on the device (agx_position_searcher_*): the pool's slots take boards off a list instead of openings, search each
	 * as a fresh GameGenerator would search for its first move (empty tree, empty solver table, generation 1, nn_queued 0), and hand the
	 * root over when the move rule of k_expand fires — nothing is played.  k_load_positions is the front end (begin_game's work, from a
	 * board), k_harvest_positions the back end (k_advance's place in the step: final selector, dense per-cell rows, principal variation),
	 * and a harvested slot is left as a finished game is, so that k_arena_service takes grown arenas back before the next load.
	 */
	/* every output of position p that has no root behind it: zeros, no edge anywhere (whole workgroup of `threads`) */
	__device__ void position_write_empty(const PositionJob &J, int p, int hw, int status, int nodes, int edges, int steps, int error, int tid, int threads)
	{
		const AgxPositionSearchOutputs &o = J.out;
		const size_t row = static_cast<size_t>(p) * hw;
		for (int i = tid; i < hw; i += threads)
		{
			if (o.visits != nullptr)
				o.visits[row + i] = 0;
			if (o.prior != nullptr)
				o.prior[row + i] = 0.0f;
			if (o.q != nullptr)
			{
				o.q[2 * (row + i)] = 0.0f;
				o.q[2 * (row + i) + 1] = 0.0f;
			}
			if (o.score != nullptr)
				o.score[row + i] = 0;
			if (o.edge_index != nullptr)
				o.edge_index[row + i] = -1;
		}
		if (o.pv != nullptr)
			for (int i = tid; i < J.max_pv; i += threads)
				o.pv[static_cast<size_t>(p) * J.max_pv + i] = 0;
		if (tid == 0)
		{
			if (J.sink.d_bytes != nullptr && J.sink.d_sizes != nullptr)
				J.sink.d_sizes[p] = 0; // no root, no sample: the bytes stay as they are
			if (o.status != nullptr)
				o.status[p] = status;
			if (o.root != nullptr)
				o.root[4 * p] = o.root[4 * p + 1] = o.root[4 * p + 2] = o.root[4 * p + 3] = 0;
			if (o.root_value != nullptr)
				o.root_value[2 * p] = o.root_value[2 * p + 1] = 0.0f;
			if (o.best_move != nullptr)
				o.best_move[p] = 0;
			if (o.pv_length != nullptr)
				o.pv_length[p] = 0;
			if (o.info != nullptr)
			{
				o.info[4 * p] = nodes;
				o.info[4 * p + 1] = edges;
				o.info[4 * p + 2] = steps;
				o.info[4 * p + 3] = error;
			}
		}
	}
	__global__ __launch_bounds__(64) void k_positions_init(EngineDev E, PositionJob J)
	{ // what k_begin does for a pool without openings: every slot idle and free, counting from zero
		const int g = blockIdx.x;
		if (threadIdx.x != 0)
			return;
		GameState &gs = E.games[g];
		gs.generation = 0;
		gs.error = 0;
		gs.games_done = 0;
		gs.arena = 0;
		for (int i = 0; i < 12; i++)
			gs.stats[i] = 0;
		gs.active = 0;
		gs.root = -1;
		gs.n_nodes = 0;
		gs.n_edges = 0;
		gs.n_tasks = 0;
		gs.need_move = 0;
		gs.solve_pos = 0;
		gs.solve_pending = 0;
		gs.outcome = 0;
		gs.n_moves = 0;
		gs.restart_id = -1;
		J.slot_position[g] = -1;
		J.slot_steps[g] = 0;
		if (g == 0)
		{
			*J.cursor = 0;
			*J.finished = 0;
		}
	}
	__global__ void k_positions_reset(PositionJob J)
	{ // a new list: every slot is free (the previous job has finished)
		*J.cursor = 0;
		*J.finished = 0;
	}
	/* A free slot takes the next position of the list: a sibling of begin_game, from a board.  Tree::clear + AlphaBetaSearch::clear, a new
	 * AlphaBetaSearch's generation (0, prepare_search makes it 1), the board with its stones as a move list in cell order, nn_queued 0, the
	 * caller's serial where a game has its opening id.  A position that is none (k_encode_positions' rule) gets status 1 and the slot goes on
	 * to the next one.  One workgroup of 256 threads per slot. */
	__global__ __launch_bounds__(256) void k_load_positions(EngineDev E, PositionJob J)
	{
		__shared__ u64 scratch[4];
		__shared__ int sh_p, sh_bad, sh_count;
		const int g = E.g0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, hw = E.hw;
		if (J.slot_position[g] >= 0)
			return;
		GameState &gs = E.games[g];
		const uint8_t *src = nullptr;
		int p = -1, sign = 0;
		while (true)
		{
			if (tid == 0)
			{
				int next = -1;
				if (__hip_atomic_load(J.cursor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < J.n)
				{
					next = atomicAdd(J.cursor, 1);
					if (next >= J.n)
						next = -1;
				}
				sh_p = next;
				sh_bad = 0;
			}
			__syncthreads();
			p = sh_p;
			if (p < 0)
				return; // the list is used up: the slot stays free
			src = J.boards + static_cast<size_t>(p) * hw;
			sign = J.signs[p];
			bool bad = (sign != 1 && sign != 2);
			for (int i = tid; i < hw; i += 256)
				bad |= (src[i] > 2);
			if (bad)
				sh_bad = 1;
			__syncthreads();
			if (!sh_bad)
				break;
			position_write_empty(J, p, hw, AGX_POSSEARCH_STATUS_BAD_INPUT, 0, 0, 0, 0, tid, 256);
			if (tid == 0)
				atomicAdd(J.finished, 1);
			__syncthreads();
		}
		clear_tree_and_table(E, g, tid);
		for (int k = tid; k < E.batch; k += 256)
		{ // a new GameGenerator's Search has new SearchTasks: what survives SearchTask::set (the solved flags, moves_left) must not come from the slot's previous position
			DTask &t = E.tasks[static_cast<size_t>(g) * E.batch + k];
			t.path_len = 0;
			t.final_node = 0;
			t.n_edges = 0;
			t.flags = 0;
			t.sign_to_move = 0;
			t.score = 0;
			t.win = 0.0f;
			t.draw = 0.0f;
			t.moves_left = 0.0f;
			t.needs_nn = 0;
			t.symmetry = 0;
		}
		for (int i = tid; i < hw; i += 256)
			gs.board[i] = src[i];
		if (tid < BWORDS)
		{
			u64 w = 0;
			for (int c = 0; c < 32; c++)
			{
				const int cell = 32 * tid + c;
				if (cell < hw)
					w |= static_cast<u64>(src[cell]) << (2 * c);
			}
			gs.cboard[tid] = w;
		}
		if (tid < 64)
		{ // the stones as moves, in cell order (up to hw of them)
			int count = 0;
			for (int base = 0; base < hw; base += 64)
			{
				const int i = base + lane;
				const uint32_t v = (i < hw) ? src[i] : 0u;
				const u64 m = __ballot(v != 0u);
				if (v != 0u)
					gs.moves[count + __popcll(m & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))))] = static_cast<uint16_t>(v | (static_cast<uint32_t>(i / E.n) << 2) | (static_cast<uint32_t>(i % E.n) << 9));
				count += __popcll(m);
			}
			if (lane == 0)
				sh_count = count;
		}
		__syncthreads();
		if (tid == 0)
		{
			gs.sign_to_move = sign;
			gs.n_moves = sh_count;
			gs.outcome = 0;
			gs.root = -1;
			gs.n_nodes = 0;
			gs.n_edges = 0;
			gs.n_tasks = 0;
			gs.need_move = 0;
			gs.solve_pos = 0;
			gs.solve_pending = 0;
			park_forget_game(E, g);
			gs.grow_pending = 0;
			gs.max_depth = 0;
			gs.nn_queued = 0;
			gs.restart_id = 0;
			gs.noise_ready = 0;
			gs.generation = 1; // a new AlphaBetaSearch counts from 0, prepare_search -> increaseGeneration
			gs.opening_id = (J.serials != nullptr) ? J.serials[p] : 0;
			gs.error = 0;
			gs.arena = 0;
			gs.active = 1;
		}
		__syncthreads();
		u64 h = 0;
		for (int i = tid; i < hw; i += 256)
			h ^= E.nc_keys[3 + 3 * i + gs.board[i]];
		block_reduce_xor(h, scratch, tid);
		if (tid == 0)
		{
			gs.root_hash = h ^ E.nc_keys[sign];
			J.slot_steps[g] = 0;
			J.slot_position[g] = p;
		}
	}
	/* the rating of cfg.final_selector for one root edge: k_advance's switch, the same arithmetic (EdgeSelector.cpp:446-536) */
	__device__ __forceinline__ float final_selector_rating(const EngineDev &E, const DEdge &e, const DNode &root)
	{
		switch (E.final_selector)
		{
			default:
				return best_edge_rating(e, root);
			case 1:
				return e.visits;
			case 2:
				return -e.visits;
			case 3:
				switch (s_pv(e.score))
				{
					case 0:
						return -1000.0f + s_distance(e.score);
					case 1:
						return 0.5f; // Value::draw().getExpectation()
					case 3:
						return +1000.0f - s_distance(e.score);
					default:
						return e.win + 0.5f * e.draw;
				}
			case 4:
				return e.prior;
			case 5:
			{ // LCB (EdgeSelector.cpp:446-475)
				const int pv = s_pv(e.score);
				if (pv == 0)
					return -1.0e6f + s_distance(e.score) + e.prior;
				if (pv == 3)
					return +1.0e6f - s_distance(e.score) + e.prior;
				const int vl = e.flag_vl & 0x7FFF;
				const float visits = 1.0e-8f + e.visits;
				const float vl_factor = visits / (visits + static_cast<float>(vl));
				const float Q = (e.visits > 0) ? (e.win + 0.5f * e.draw) : (root.win + 0.5f * root.draw);
				const float parent_log_visit = static_cast<float>(det_log(static_cast<double>(root.visits + root.vl)));
				const float U = E.c_puct * sqrtf(parent_log_visit / (1.0f + e.visits + vl));
				return Q * vl_factor - U;
			}
		}
	}
	/* The root of position p as the reference's SearchDataStorage_v201 bytes (sample_v201.hpp): k_advance's quantiser (SearchDataPack of the
	 * root -> loadFrom + serialize, dataset/SearchDataStorage.cpp:326-374,410-419) for one wave, on the cell -> edge map of the harvest
	 * stage.  The three maxima go through wave reductions (non-negative floats order like their bits); the kept cells — an edge with visits
	 * or a proven score — are compacted in cell order by ballots, 64 cells at a time; on boards of more than 255 cells, where a cell 255 or
	 * more past the previous entry gets an entry too, lane 0 walks the ballots' words instead (at most 400 cells).  entry_cell: LDS of the
	 * caller, [MAXHW]; kept: [(MAXHW + 63) / 64]. */
	__device__ void position_write_sample(const PositionJob &J, int p, const GameState &gs, const DNode &root, const DEdge *edges, const int16_t *cell_edge,
			uint16_t *entry_cell, u64 *kept, int *sh_count, int hw, int lane)
	{
		const int n_edges = root.n_edges;
		uint32_t max_prior = 0u, max_value = 0u, max_visits = 0u;
		for (int i = lane; i < n_edges; i += 64)
		{
			const DEdge e = edges[root.edge_begin + i];
			const float wd = fmaxf(e.win, e.draw);
			max_prior = max(max_prior, __float_as_uint((e.prior > 0.0f) ? e.prior : 0.0f));
			max_value = max(max_value, __float_as_uint((wd > 0.0f) ? wd : 0.0f));
			max_visits = max(max_visits, static_cast<uint32_t>(max(e.visits, 0)));
		}
		max_prior = wave_reduce_umax(max_prior);
		max_value = wave_reduce_umax(max_value);
		max_visits = wave_reduce_umax(max_visits);
		const float prior_scale = v201::prior_scale(__uint_as_float(max_prior)), value_scale = v201::value_scale(__uint_as_float(max_value));
		const float visit_scale = v201::visit_scale(fmaxf(1.0f, static_cast<float>(max_visits)));
		// ---- which cells get an entry (:333-337, in cell order) ----
		int count = 0;
		for (int base = 0; base < hw; base += 64)
		{
			const int i = base + lane;
			bool natural = false;
			if (i < hw && cell_edge[i] >= 0)
			{
				const DEdge e = edges[root.edge_begin + cell_edge[i]];
				natural = e.visits > 0 || s_proven(e.score);
			}
			const u64 m = __ballot(natural);
			if (hw <= 255)
			{ // no cell can be 255 past anything: the entries are the kept cells
				if (natural)
					entry_cell[count + __popcll(m & ((lane == 0) ? 0ull : (~0ull >> (64 - lane))))] = static_cast<uint16_t>(i);
				count += __popcll(m);
			}
			else if (lane == 0)
				kept[base >> 6] = m;
		}
		if (hw > 255)
		{
			if (lane == 0)
			{
				int last = 0;
				for (int i = 0; i < hw; i++)
					if (((kept[i >> 6] >> (i & 63)) & 1ull) || (i - last) >= 255)
					{
						entry_cell[count++] = static_cast<uint16_t>(i);
						last = i;
					}
				*sh_count = count;
			}
			__syncthreads();
			count = *sh_count;
		}
		__syncthreads();
		// ---- header and entries; byte stores: the sink's address need not be aligned beyond the caller's stride ----
		uint8_t *out = J.sink.d_bytes + static_cast<size_t>(p) * static_cast<size_t>(J.sink.stride);
		if (lane < v201::HEADER_BYTES)
		{
			uint32_t word; // the 16 header bytes as four little-endian words
			switch (lane >> 2)
			{
				case 0: word = v201::ScaleFormat::encode(value_scale) | (v201::ScaleFormat::encode(prior_scale) << 16); break;
				case 1: word = v201::ScaleFormat::encode(visit_scale) | (static_cast<uint32_t>(root.score & 0xFFFFu) << 16); break;
				case 2: word = static_cast<uint32_t>(gs.n_moves & 0xFFFF) | (static_cast<uint32_t>((root.flags >> 3) & 7) << 16); break; // stones on the board the root stands for
				default: word = static_cast<uint32_t>(count); break;
			}
			out[lane] = static_cast<uint8_t>(word >> (8 * (lane & 3)));
		}
		for (int k = lane; k < count; k += 64)
		{
			const int cell = entry_cell[k], previous = (k > 0) ? entry_cell[k - 1] : 0;
			const int ei = cell_edge[cell];
			int visits = 0;
			float prior = 0.0f, win = 0.0f, draw = 0.0f;
			uint32_t score = s_unknown(0); // a filler cell without an edge: the SearchDataPack defaults (Score(), Value())
			if (ei >= 0)
			{
				const DEdge e = edges[root.edge_begin + ei];
				visits = e.visits;
				prior = e.prior;
				win = e.win;
				draw = e.draw;
				score = e.score;
			}
			uint8_t *q = out + v201::HEADER_BYTES + v201::ENTRY_BYTES * k;
			q[0] = static_cast<uint8_t>(cell - previous);
			q[1] = static_cast<uint8_t>(v201::VisitFormat::encode(static_cast<float>(visits) / visit_scale));
			q[2] = static_cast<uint8_t>(v201::PriorFormat::encode(prior / prior_scale));
			q[3] = static_cast<uint8_t>(v201::score_code(score));
			q[4] = static_cast<uint8_t>(v201::PriorFormat::encode(win / value_scale));
			q[5] = static_cast<uint8_t>(v201::PriorFormat::encode(draw / value_scale));
		}
		if (lane == 0)
			J.sink.d_sizes[p] = v201::HEADER_BYTES + v201::ENTRY_BYTES * count;
	}
	/* k_advance's place in a step of the position searcher, one wave per slot: a slot whose move rule has fired (or whose engine error word is
	 * set, or that has spent max_steps steps) writes the outputs of its position and becomes a finished game: leaves still in flight give their
	 * virtual losses back (k_cancel_pending), park buffers are forgotten, grown arenas wait for k_arena_service, the slot is free. */
	__global__ __launch_bounds__(64) void k_harvest_positions(EngineDev E, PositionJob J)
	{
		__shared__ u64 sh_cboard[BWORDS];
		__shared__ int16_t cell_edge[MAXHW];
		__shared__ uint16_t entry_cell[MAXHW]; // (the sample sink's: position_write_sample)
		__shared__ u64 kept_cells[(MAXHW + 63) / 64];
		__shared__ int sh_entries;
		const int g = E.g0 + blockIdx.x, lane = threadIdx.x, hw = E.hw, n = E.n;
		const int p = J.slot_position[g];
		if (p < 0)
			return;
		GameState &gs = E.games[g];
		const int steps = J.slot_steps[g] + 1, error = gs.error;
		const bool searched = gs.active && gs.need_move && !gs.solve_pending && !gs.grow_pending && error == 0;
		if (!searched && error == 0 && steps < J.max_steps)
		{
			if (lane == 0)
				J.slot_steps[g] = steps;
			return;
		}
		const int status = searched ? 0 : ((error != 0) ? AGX_POSSEARCH_STATUS_ENGINE_ERROR : AGX_POSSEARCH_STATUS_STEP_LIMIT);
		use_game_arenas(E, g);
		DNode *nodes = nodes_of(E, g, gs.arena);
		DEdge *edges = edges_of(E, g, gs.arena);
		if (status == AGX_POSSEARCH_STATUS_STEP_LIMIT)
		{ // Search::cleanup: the batch in flight (waiting for its solver, or for larger arenas) is dropped, the root stands without its virtual losses
			const int pending = gs.n_tasks;
			for (int k = 0; k < pending; k++)
			{
				const DTask &t = E.tasks[static_cast<size_t>(g) * E.batch + k];
				cancel_virtual_loss(nodes, edges, t, t.path_len, lane);
				wave_sync();
			}
			__threadfence_block();
			__syncthreads();
		}
		const AgxPositionSearchOutputs &o = J.out;
		const bool have_root = status != AGX_POSSEARCH_STATUS_ENGINE_ERROR && gs.root >= 0; // (a tree that stopped on an error is not read)
		if (!have_root)
			position_write_empty(J, p, hw, status, gs.n_nodes, gs.n_edges, steps, error, lane, 64);
		else
		{
			DNode root;
			node_head(root, nodes[gs.root]);
			const int n_edges = root.n_edges;
			for (int i = lane; i < hw; i += 64)
				cell_edge[i] = -1;
			__syncthreads();
			// ---- final selector: k_advance's rule — first strict maximum per lane, then the lowest index among the lanes' maxima ----
			float best_value = -3.402823466e+38f;
			int best = 0x7FFFFFFF;
			for (int i = lane; i < n_edges; i += 64)
			{ // (a root on an empty 20x20 board has 400 edges)
				const DEdge e = edges[root.edge_begin + i];
				cell_edge[((e.move >> 2) & 127) * n + ((e.move >> 9) & 127)] = static_cast<int16_t>(i);
				const float value = final_selector_rating(E, e, root);
				if (value > best_value)
				{
					best_value = value;
					best = i;
				}
			}
			wave_argmax(best_value, best);
			__syncthreads();
			const size_t row = static_cast<size_t>(p) * hw;
			for (int i = lane; i < hw; i += 64)
			{
				const int ei = cell_edge[i];
				DEdge e;
				e.prior = e.win = e.draw = 0.0f;
				e.visits = 0;
				e.score = 0;
				if (ei >= 0)
					e = edges[root.edge_begin + ei];
				if (o.visits != nullptr)
					o.visits[row + i] = e.visits;
				if (o.prior != nullptr)
					o.prior[row + i] = e.prior;
				if (o.q != nullptr)
				{
					o.q[2 * (row + i)] = e.win;
					o.q[2 * (row + i) + 1] = e.draw;
				}
				if (o.score != nullptr)
					o.score[row + i] = e.score;
				if (o.edge_index != nullptr)
					o.edge_index[row + i] = static_cast<int16_t>(ei);
			}
			if (lane == 0)
			{
				if (o.status != nullptr)
					o.status[p] = status;
				if (o.root != nullptr)
				{
					o.root[4 * p] = root.visits;
					o.root[4 * p + 1] = root.score;
					o.root[4 * p + 2] = (root.flags >> 3) & 7; // DNode flags 8 / 16 / 32, as AgxMoveRecord.root_flags
					o.root[4 * p + 3] = n_edges;
				}
				if (o.root_value != nullptr)
				{
					o.root_value[2 * p] = root.win;
					o.root_value[2 * p + 1] = root.draw;
				}
				if (o.best_move != nullptr)
					o.best_move[p] = (best < n_edges) ? edges[root.edge_begin + best].move : static_cast<uint16_t>(0);
				if (o.info != nullptr)
				{
					o.info[4 * p] = gs.n_nodes;
					o.info[4 * p + 1] = gs.n_edges;
					o.info[4 * p + 2] = steps;
					o.info[4 * p + 3] = error;
				}
			}
			if (J.sink.d_bytes != nullptr && J.sink.d_sizes != nullptr) // (uniform: the job's)
				position_write_sample(J, p, gs, root, edges, cell_edge, entry_cell, kept_cells, &sh_entries, hw, lane);
			// ---- the principal variation: k_principal_variation's walk from the root ----
			const int *ht = ht_of(E, g);
			QueryWalk q;
			query_begin(E, gs, sh_cboard, q, lane);
			int length = 0;
			while (length < J.max_pv)
			{
				const int found = q.valid ? cache_seek(E, nodes, ht, q.hash, sh_cboard, q.sign, lane) : -1;
				if (found < 0)
					break;
				DNode nd;
				node_head(nd, nodes[found]);
				if (nd.n_edges <= 0)
					break;
				float pv_value = -3.402823466e+38f;
				int pv_best = 0x7FFFFFFF;
				for (int i = lane; i < nd.n_edges; i += 64)
				{
					const float value = best_edge_rating(edges[nd.edge_begin + i], nd);
					if (value > pv_value)
					{
						pv_value = value;
						pv_best = i;
					}
				}
				wave_argmax(pv_value, pv_best);
				if (pv_best >= nd.n_edges)
					break;
				const uint16_t move = edges[nd.edge_begin + pv_best].move;
				if (lane == 0 && o.pv != nullptr)
					o.pv[static_cast<size_t>(p) * J.max_pv + length] = move;
				query_place(E, sh_cboard, q, move, lane);
				length++;
			}
			if (o.pv != nullptr)
				for (int i = length + lane; i < J.max_pv; i += 64)
					o.pv[static_cast<size_t>(p) * J.max_pv + i] = 0;
			if (lane == 0 && o.pv_length != nullptr)
				o.pv_length[p] = length;
		}
		__syncthreads();
		if (lane == 0)
		{ // a finished game: nothing in flight, waiting (restart_id -1) — k_arena_service takes a grown bundle back, k_load_positions the slot
			gs.active = 0;
			gs.need_move = 0;
			gs.n_tasks = 0;
			gs.solve_pos = 0;
			gs.solve_pending = 0;
			park_forget_game(E, g);
			gs.grow_pending = 0;
			gs.root = -1;
			gs.restart_id = -1;
			gs.games_done++;
			J.slot_steps[g] = steps;
			J.slot_position[g] = -1;
			atomicAdd(J.finished, 1);
		}
	}

	/* debug / test kernels --------------------------------------------------------------------------------------- */
	__global__ __launch_bounds__(64) void k_debug_load_tasks(EngineDev E, const uint8_t *boards, const int *signs, int count)
	{ // makes every game look as if one fresh leaf had been selected: task 0 = given position
		const int g = blockIdx.x, lane = threadIdx.x;
		if (g >= count)
			return;
		GameState &gs = E.games[g];
		DTask &t = E.tasks[static_cast<size_t>(g) * E.batch];
		for (int i = lane; i < E.hw; i += 64)
			t.board[i] = boards[static_cast<size_t>(g) * E.hw + i];
		if (lane == 0)
		{
			t.path_len = 1;
			t.final_node = -1;
			t.n_edges = 0;
			t.flags = 0;
			t.sign_to_move = signs[g];
			t.score = s_unknown(0);
			t.needs_nn = 0;
			gs.n_tasks = 1;
			gs.active = 1;
			gs.outcome = 0;
			gs.error = 0;
			gs.solve_pos = 0; // (gs.generation: the idle template's — 0 until agx_debug_new_generation)
			gs.solve_pending = 0;
			park_forget_game(E, g);
			gs.nn_queued = 0;
		}
	}
	/* ------------------------------------------------------------------------------------------------------------ */
	/*
	 * k_solve_positions — the threat solver on a batch of boards (agx_position_solver_solve): every position as a fresh AlphaBetaSearch with an
	 * empty table would solve it.  One wavefront per position, grid-stride: wave w owns table w, spill area w, task w and game record w of a
	 * minimal EngineDev (tt_mod = the wave count), clears its table, loads the position into its task and runs solve_task on it — the loop
	 * around solver_run / solver_place is that function's.  Nothing is shared between waves: no atomics, no waiting; a solve ends by its node
	 * budget and solve_task's depth loop.
	 */
	template<bool RENJU, int NFIX>
	__global__ __launch_bounds__(64, AGX_SOLVE_WAVES) void k_solve_positions(EngineDev E, SolvePositionsArgs A)
	{
		if (NFIX != 0)
		{
			E.n = NFIX;
			E.hw = NFIX * NFIX;
		}
		typedef SolverSharedT<(NFIX != 0) ? NFIX : MAXN> SH;
		__shared__ SH sh;
		const int w = blockIdx.x, lane = threadIdx.x, hw = E.hw;
		DTask &t = E.tasks[w];
		GameState &gs = E.games[w];
		ulonglong2 *tt = reinterpret_cast<ulonglong2*>(E.tt + static_cast<size_t>(w) * (E.tt_bucket_mask + 1ull) * 8ull);
		const size_t entries = (E.tt_bucket_mask + 1ull) * 4ull;
		solver_load_threat_table(sh, E, lane);
		for (int p = w; p < A.n; p += gridDim.x)
		{
			const uint8_t *src = A.boards + static_cast<size_t>(p) * hw;
			const int sign = A.signs[p];
			bool bad = false;
			for (int i = lane; i < hw; i += 64)
			{
				const uint8_t v = src[i];
				bad |= (v > 2);
				t.board[i] = v;
			}
			// not a position: nothing of it reaches the solver, whose tables are indexed by cell values (the rule of k_encode_positions)
			const bool refused = __ballot(bad) != 0ull || (sign != 1 && sign != 2);
			int status = AGX_POSSOLVE_STATUS_BAD_INPUT, size = 0;
			uint32_t score = 0, flags = 0, nodes = 0;
			if (!refused)
			{
				ulonglong2 empty;
				empty.x = 0ull;
				empty.y = tt_pack(0, 0, s_unknown(0), 0);
				for (size_t i = lane; i < entries; i += 64)
					tt[i] = empty;
				if (lane == 0)
				{ // one fresh leaf, as k_debug_load_tasks makes it
					t.path_len = 1;
					t.final_node = -1;
					t.n_edges = 0;
					t.flags = 0;
					t.sign_to_move = sign;
					t.score = s_unknown(0);
					t.win = t.draw = t.moves_left = 0.0f;
					t.needs_nn = 0;
					gs.error = 0;
				}
				__threadfence(); // the board, the task and the empty table are read back by other lanes
				wave_sync();
				unsigned long long solver_nodes = 0;
				solve_task<RENJU>(sh, E, w, t, w, 0, lane, solver_nodes, w);
				__threadfence(); // lane 0 wrote the task's words and the game's error
				wave_sync();
				size = __builtin_amdgcn_readfirstlane(t.n_edges);
				score = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(t.score)));
				flags = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(t.flags)));
				nodes = static_cast<uint32_t>(solver_nodes);
				status = (__builtin_amdgcn_readfirstlane(gs.error) != 0) ? AGX_POSSOLVE_STATUS_SOLVER_ERROR : 0;
			}
			for (int i = lane; i < hw; i += 64)
			{ // the whole row, zeros behind the list: the outputs are a function of the position alone
				if (A.out.moves != nullptr)
					A.out.moves[static_cast<size_t>(p) * hw + i] = (i < size) ? t.emove[i] : static_cast<uint16_t>(0);
				if (A.out.move_scores != nullptr)
					A.out.move_scores[static_cast<size_t>(p) * hw + i] = (i < size) ? t.escore[i] : static_cast<uint16_t>(0);
			}
			if (lane < 3 && A.out.value != nullptr)
			{ // Score::convertToValue of a proven score as (win, draw, loss)
				const int pv = s_pv(score);
				const bool proven = !refused && s_proven(score);
				A.out.value[static_cast<size_t>(p) * 3 + lane] = (proven && pv == ((lane == 0) ? 3 : ((lane == 1) ? 1 : 0))) ? 1.0f : 0.0f;
			}
			if (lane == 0)
			{
				if (A.out.score != nullptr)
					A.out.score[p] = static_cast<uint16_t>(score);
				if (A.out.flags != nullptr)
					A.out.flags[p] = flags;
				if (A.out.n_actions != nullptr)
					A.out.n_actions[p] = size;
				if (A.out.nodes != nullptr)
					A.out.nodes[p] = nodes;
				if (A.out.status != nullptr)
					A.out.status[p] = status;
			}
			wave_sync(); // the next position reuses the task and the LDS state
		}
	}

	__global__ __launch_bounds__(64) void k_debug_pattern_state(EngineDev E, const uint8_t *boards, const int *signs, const uint16_t *moves, int n_moves,
			uint8_t *ptypes, uint8_t *threats, int16_t *lists, int lists_stride)
	{
		__shared__ SolverShared sh;
		const int g = blockIdx.x, lane = threadIdx.x;
		if (lane == 0)
		{
			sh.spill_lists = E.list_spill + static_cast<size_t>(g) * 20 * MAXHW;
			sh.spill_frames = reinterpret_cast<Frame*>(E.frame_spill) + static_cast<size_t>(g) * MAX_FRAMES;
			sh.snap = E.snap_spill + static_cast<size_t>(g) * (E.hw + 2) * 64;
		}
		solver_load_threat_table(sh, E, lane);
		solver_set_board(sh, E, boards + static_cast<size_t>(g) * E.hw, signs[g], lane);
		__shared__ uint16_t done[512];
		__shared__ int n_done;
		if (lane == 0)
			n_done = 0;
		__syncthreads();
		for (int i = 0; i < n_moves; i++)
		{
			const uint32_t m = moves[static_cast<size_t>(g) * n_moves + i];
			if (m == 0xFFFFu)
				continue;
			if ((m & 3) == 0)
			{
				const uint32_t u = done[n_done - 1];
				solver_place(sh, E, u, false, lane);
				if (lane == 0)
					n_done--;
			}
			else
			{
				solver_place(sh, E, m, true, lane);
				if (lane == 0)
					done[n_done++] = static_cast<uint16_t>(m);
			}
			__syncthreads();
		}
		for (int i = lane; i < E.hw; i += 64)
		{
			for (int k = 0; k < 8; k++)
				ptypes[(static_cast<size_t>(g) * E.hw + i) * 8 + k] = sh.ptype[i][k];
			threats[(static_cast<size_t>(g) * E.hw + i) * 2] = sh.threat[i][0];
			threats[(static_cast<size_t>(g) * E.hw + i) * 2 + 1] = sh.threat[i][1];
		}
		if (lane == 0)
		{
			int16_t *out = lists + static_cast<size_t>(g) * lists_stride;
			int pos = 0;
			for (int s = 0; s < 2; s++)
				for (int t = 0; t < 10; t++)
				{
					out[pos++] = static_cast<int16_t>(sh.count[s][t]);
					if (t == 1)
					{ // HALF_OPEN_3: only the size is kept on the device; the cells are listed in row-major order (the caller compares them as a set)
						for (int cell = 0; cell < E.hw; cell++)
							if (sh.threat[cell][s] == 1)
							{
								out[pos++] = static_cast<int16_t>(cell / E.n);
								out[pos++] = static_cast<int16_t>(cell % E.n);
							}
						continue;
					}
					for (int k = 0; k < sh.count[s][t]; k++)
					{
						const int cell = (t == 0) ? 0 : static_cast<int>(list_get(sh, s, t, k));
						out[pos++] = static_cast<int16_t>(cell / E.n);
						out[pos++] = static_cast<int16_t>(cell % E.n);
					}
				}
			out[lists_stride - 1] = static_cast<int16_t>(pos);
		}
	}
}

/* ================================================================================================================ */
/* The launch layer (engine_launch.hpp): what the host files call.  Nothing below knows AgxEngine or the C ABI. */

#if defined(AGX_QUICK) && !defined(AGX_QUICK_RENJU)
#define AGX_QUICK_RENJU false /* developer builds (AGX_QUICK: only the 15x15 solver is instantiated); -DAGX_QUICK_RENJU=true: the renju solver instead of the other rules' */
#endif
/* (rules, board size) -> the compile-time pair {renju, NFIX} of k_search_spec, k_solve and k_solve_positions: USE(RENJU, NFIX) is expanded
 * for the one shape that plays these rules on this board (NFIX 15 and 20 are the boards with kernels of their own, 0 is any size) */
#ifdef AGX_QUICK /* developer builds: one shape only, the 15x15 board (a fifth of the compile time) */
#define AGX_FOR_SHAPE(rules, n, USE) do { (void) (rules); (void) (n); USE(AGX_QUICK_RENJU, 15); } while (0)
#else
#define AGX_FOR_SHAPE(rules, n, USE) \
	do { \
		if ((rules) == AGX_RENJU) \
		{ \
			if ((n) == 15) \
				USE(true, 15); \
			else \
				USE(true, 0); \
		} \
		else if ((n) == 15) \
			USE(false, 15); \
		else if ((n) == 20) \
			USE(false, 20); \
		else \
			USE(false, 0); \
	} while (0)
#endif

namespace agx_eng
{
	/* the instantiation of k_search_spec a pool of these rules and board size launches; merged: the variant for a match pool's launch over
	 * both players' trees (k_search_spec's MERGED) */
	typedef void (*SpecKernel)(EngineDev, int);
	static SpecKernel spec_kernel(int rules, int n, bool merged)
	{
		SpecKernel kernel = nullptr;
#define AGX_USE(RENJU, NFIX) kernel = merged ? k_search_spec<RENJU, NFIX, true> : k_search_spec<RENJU, NFIX, false>
		AGX_FOR_SHAPE(rules, n, AGX_USE);
#undef AGX_USE
		return kernel;
	}
	int spec_resident_waves_per_cu(int rules, int n)
	{
		int blocks = 0;
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, reinterpret_cast<const void*>(spec_kernel(rules, n, false)), 64, 0) != hipSuccess || blocks <= 0)
		{
			(void) hipGetLastError();
			return 12;
		}
		return blocks;
	}
	void search_spec(const EngineDev &d, int count, hipStream_t s)
	{
		hipLaunchKernelGGL(spec_kernel(d.rules, d.n, d.match_merged != 0), dim3(d.spec_waves), dim3(64), 0, s, d, count);
	}
	void begin(const EngineDev &d, hipStream_t s)
	{
		hipLaunchKernelGGL(k_begin, dim3(d.n_games), dim3(256), 0, s, d);
	}
	void assign_openings(const EngineDev &d, int count, hipStream_t s)
	{
		hipLaunchKernelGGL(k_assign_openings, dim3(1), dim3(1024), 0, s, d, count);
	}
	void match_restart(const EngineDev &d, int pairs, hipStream_t s)
	{
		hipLaunchKernelGGL(k_match_restart, dim3(pairs), dim3(256), 0, s, d);
	}
}

extern "C" __global__ void k_reset_spec(int *nn_counter, int *nn_second, int *spec_counters, int *done_counter) // (its unmangled name is in the committed traces)
{
	*nn_counter = 0;
	*done_counter = 0;
	if (nn_second != nullptr)
		*nn_second = 0;
	for (int i = 0; i < 4; i++)
		spec_counters[i] = 0;
}

namespace agx_eng
{
	void reset_spec(int *nn_counter, int *nn_second, int *spec_counters, int *done_counter, hipStream_t s)
	{
		hipLaunchKernelGGL(k_reset_spec, dim3(1), dim3(1), 0, s, nn_counter, nn_second, spec_counters, done_counter);
	}
	void solve(const EngineDev &d, int count, bool with_select, hipStream_t s)
	{
		const dim3 grid(count), block(64);
#define AGX_USE_FUSED(RENJU, NFIX) hipLaunchKernelGGL((k_solve<RENJU, NFIX, true>), grid, block, 0, s, d)
#define AGX_USE_SPLIT(RENJU, NFIX) hipLaunchKernelGGL((k_solve<RENJU, NFIX, false>), grid, block, 0, s, d)
		if (with_select)
			AGX_FOR_SHAPE(d.rules, d.n, AGX_USE_FUSED);
		else
			AGX_FOR_SHAPE(d.rules, d.n, AGX_USE_SPLIT);
#undef AGX_USE_FUSED
#undef AGX_USE_SPLIT
	}
	void reset_counter(int *counter, int *second, hipStream_t s)
	{
		hipLaunchKernelGGL(k_reset_counter, dim3(1), dim3(1), 0, s, counter, second);
	}
	void select(const EngineDev &d, int waves, hipStream_t s)
	{
		hipLaunchKernelGGL(k_select, dim3(waves), dim3(64), 0, s, d);
	}
	void expand_merged(const EngineDev &d, hipStream_t s)
	{
		hipLaunchKernelGGL(k_expand<true>, dim3(d.n_games), dim3(64), 0, s, d);
	}
	void advance_merged(const EngineDev &d, hipStream_t s)
	{
		hipLaunchKernelGGL(k_advance<true>, dim3(d.n_games), dim3(ADV_THREADS), 0, s, d);
	}
	void match_pair_log(const EngineDev &d, const PairLogDev &log, hipStream_t s)
	{
		hipLaunchKernelGGL(k_match_pair_log, dim3(1), dim3(256), 0, s, d, log);
	}
	void arena_service(const EngineDev &d, int count, int assign_count, hipStream_t s)
	{
		hipLaunchKernelGGL(k_arena_service, dim3(1), dim3(1024), 0, s, d, count, assign_count);
	}
	void arena_copy(const EngineDev &d, int trees, hipStream_t s)
	{
		hipLaunchKernelGGL(k_arena_copy, dim3(trees * CLEAR_PARTS), dim3(256), 0, s, d, CLEAR_PARTS);
	}
	void clear_tables(const EngineDev &d, int games, int restart, hipStream_t s)
	{
		hipLaunchKernelGGL(k_clear_tables, dim3(games * CLEAR_PARTS), dim3(256), 0, s, d, CLEAR_PARTS, restart);
	}
	void expand(const EngineDev &d, int waves, hipStream_t s)
	{
		hipLaunchKernelGGL(k_expand<false>, dim3(waves), dim3(64), 0, s, d);
	}
	void advance(const EngineDev &d, int trees, hipStream_t s)
	{
		hipLaunchKernelGGL(k_advance<false>, dim3(trees), dim3(ADV_THREADS), 0, s, d);
	}
	void restart(const EngineDev &d, int games, hipStream_t s)
	{
		hipLaunchKernelGGL(k_restart, dim3(games), dim3(256), 0, s, d);
	}
	void cancel_pending(const EngineDev &d, int waves, hipStream_t s)
	{
		hipLaunchKernelGGL(k_cancel_pending, dim3(waves), dim3(64), 0, s, d);
	}
	void set_board(const EngineDev &d, int g, const uint8_t *board, int sign_to_move, int force_remove_root, hipStream_t s)
	{
		hipLaunchKernelGGL(k_set_board, dim3(1), dim3(256), 0, s, d, g, board, sign_to_move, force_remove_root);
	}
	void restore_game(const EngineDev &d, int g, const uint16_t *moves, int count, int opening_id, int nn_queued, hipStream_t s)
	{
		hipLaunchKernelGGL(k_restore_game, dim3(1), dim3(256), 0, s, d, g, moves, count, opening_id, nn_queued);
	}
	void root_summary(const EngineDev &d, int g, int *out, hipStream_t s)
	{
		hipLaunchKernelGGL(k_root_summary, dim3(1), dim3(1), 0, s, d, g, out);
	}
	void node_info(const EngineDev &d, int n_paths, int tree, const uint16_t *moves, const int *offsets, AgxNodeView *out_nodes, AgxEdgeView *out_edges,
			int edges_per_path, hipStream_t s)
	{
		hipLaunchKernelGGL(k_node_info, dim3(n_paths), dim3(64), 0, s, d, tree, moves, offsets, out_nodes, out_edges, edges_per_path);
	}
	void principal_variation(const EngineDev &d, int tree, const uint16_t *moves, int n_moves, int max_length, int *out_length, uint16_t *out_pv,
			AgxEdgeView *out_edges, AgxNodeView *out_nodes, hipStream_t s)
	{
		hipLaunchKernelGGL(k_principal_variation, dim3(1), dim3(64), 0, s, d, tree, moves, n_moves, max_length, out_length, out_pv, out_edges, out_nodes);
	}
	void match_summary(const EngineDev &d, long long *out, hipStream_t s)
	{
		hipLaunchKernelGGL(k_match_summary, dim3(1), dim3(256), 0, s, d, out);
	}
	void debug_load_tasks(const EngineDev &d, const uint8_t *boards, const int *signs, int count, hipStream_t s)
	{
		hipLaunchKernelGGL(k_debug_load_tasks, dim3(count), dim3(64), 0, s, d, boards, signs, count);
	}
	void debug_pattern_state(const EngineDev &d, int count, const uint8_t *boards, const int *signs, const uint16_t *moves, int n_moves, uint8_t *ptypes,
			uint8_t *threats, int16_t *lists, int lists_stride, hipStream_t s)
	{
		hipLaunchKernelGGL(k_debug_pattern_state, dim3(count), dim3(64), 0, s, d, boards, signs, moves, n_moves, ptypes, threats, lists, lists_stride);
	}
	void solve_positions(const EngineDev &d, int waves, const SolvePositionsArgs &args, hipStream_t s)
	{
		const dim3 grid(waves), block(64);
#define AGX_USE(RENJU, NFIX) hipLaunchKernelGGL((k_solve_positions<RENJU, NFIX>), grid, block, 0, s, d, args)
		AGX_FOR_SHAPE(d.rules, d.n, AGX_USE);
#undef AGX_USE
	}
	void positions_reset(const PositionJob &job, hipStream_t s)
	{
		hipLaunchKernelGGL(k_positions_reset, dim3(1), dim3(1), 0, s, job);
	}
	void load_positions(const EngineDev &d, int slots, const PositionJob &job, hipStream_t s)
	{
		hipLaunchKernelGGL(k_load_positions, dim3(slots), dim3(256), 0, s, d, job);
	}
	void harvest_positions(const EngineDev &d, int slots, const PositionJob &job, hipStream_t s)
	{
		hipLaunchKernelGGL(k_harvest_positions, dim3(slots), dim3(64), 0, s, d, job);
	}
	void positions_init(const EngineDev &d, int slots, const PositionJob &job, hipStream_t s)
	{
		hipLaunchKernelGGL(k_positions_init, dim3(slots), dim3(64), 0, s, d, job);
	}
}
#undef AGX_FOR_SHAPE
