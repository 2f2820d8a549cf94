/*
 * engine_host.cpp — AgxEngine and the agx_engine_* / agx_debug_* entry points of the C ABI (include/agx.h): checks, allocations, copies and the
 * order of a stage's launches.  The kernels are in engine.hip; every launch here is a call of its launch layer (engine_launch.hpp, agx_eng::).
 */
#include "engine_host.hpp"
#include "tables_host.hpp"

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace agx;
using namespace agx_host;

namespace
{
	uint64_t splitmix64(uint64_t &state)
	{
		uint64_t z = (state += 0x9E3779B97F4A7C15ull);
		z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
		z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
		return z ^ (z >> 31);
	}
}

extern "C" {

int agx_engine_default_config(AgxEngineConfig *cfg)
{
	AGX_REQUIRE(cfg != nullptr, AGX_ERR_INVALID, "agx_engine_default_config: null argument");
	std::memset(cfg, 0, sizeof(*cfg));
	cfg->rules = AGX_FREESTYLE;
	cfg->board_size = 15;
	cfg->draw_after = 225;
	cfg->n_games = 1024;
	cfg->max_batch_size = 8;
	cfg->max_simulations = 400;
	cfg->exploration_constant = 1.25f;
	cfg->exploration_scaling = 0.0f;
	cfg->init_to = 0;
	cfg->information_leak_threshold = 0.01f;
	cfg->policy_expansion_threshold = 1.0e-4f;
	cfg->max_children = 0;
	cfg->tss_max_positions = 100;
	cfg->tss_table_entries = 4ull * 1024ull * 1024ull;
	cfg->zobrist_seed = 0x9E3779B97F4A7C15ull;
	cfg->node_capacity = 8192;
	cfg->edge_capacity = 524288; // whole freestyle games at 400 playouts peak at ~250 k edges per game with an untrained (flat) policy
	cfg->record_capacity = 0;
	cfg->record_edge_capacity = 0;
	cfg->solver_yield_fraction = 0.0f;
	cfg->final_selector = 0;
	cfg->use_symmetries = 0;
	cfg->symmetry_seed = 0x5DEECE66Dull;
	cfg->action_values = 0;
	cfg->match_mode = 0;
	cfg->policy_temperature = 1.0f;
	cfg->arena_reserve = 1.0f;
	cfg->search_threads = 0;
	cfg->record_format = 1;
	cfg->record_sample_capacity = 0;
	cfg->game_end_capacity = 0;
	cfg->speculative_solver = 0;
	cfg->speculative_waves = 0;
	cfg->force_expand_root = 1;
	cfg->search_buffers = 0;
	cfg->noise_type = 0;
	cfg->noise_weight = 0.0f;
	cfg->noise_seed = 0x2545F4914F6CDD1Dull;
	return AGX_OK;
}
/* a player's search settings <-> the plain fields of a launch's EngineDev (what the kernels read) */
static PlayerSearchDev player_of(const EngineDev &d)
{
	PlayerSearchDev p;
	p.max_sims = d.max_sims;
	p.batch_limit = d.batch_limit;
	p.c_puct = d.c_puct;
	p.c_scale = d.c_scale;
	p.init_to = d.init_to;
	p.leak_threshold = d.leak_threshold;
	p.expansion_threshold = d.expansion_threshold;
	p.max_children = d.max_children;
	p.policy_temperature = d.policy_temperature;
	p.tss_max_nodes = d.tss_max_nodes;
	p.final_selector = d.final_selector;
	p.has_q = d.has_q;
	return p;
}
static void use_player(EngineDev &d, const PlayerSearchDev &p)
{
	d.max_sims = p.max_sims;
	d.batch_limit = p.batch_limit;
	d.c_puct = p.c_puct;
	d.c_scale = p.c_scale;
	d.init_to = p.init_to;
	d.leak_threshold = p.leak_threshold;
	d.expansion_threshold = p.expansion_threshold;
	d.max_children = p.max_children;
	d.policy_temperature = p.policy_temperature;
	d.tss_max_nodes = p.tss_max_nodes;
	d.final_selector = p.final_selector;
	d.has_q = p.has_q;
}
/* sizing_cus > 0: nothing is allocated and no device is touched — the engine only adds up what it WOULD allocate on a device with that many
 * compute units (agx_engine_estimate_device_bytes); *out then is a host-only object for the caller to read device_bytes from and delete */
static int engine_create(const AgxEngineConfig *cfg, AgxEngine **out, int sizing_cus)
{
	AGX_REQUIRE(cfg != nullptr && out != nullptr, AGX_ERR_INVALID, "agx_engine_create: null argument");
	AGX_REQUIRE(cfg->rules >= 0 && cfg->rules <= AGX_CARO6, AGX_ERR_INVALID, "agx_engine_create: unknown rules %d", cfg->rules);
	AGX_REQUIRE(cfg->board_size >= 5 && cfg->board_size <= MAXN, AGX_ERR_UNSUPPORTED, "agx_engine_create: board size %d not in [5, %d]", cfg->board_size, MAXN);
	AGX_REQUIRE(cfg->n_games > 0 && cfg->max_batch_size > 0 && cfg->max_simulations > 0, AGX_ERR_INVALID, "agx_engine_create: non-positive sizes");
	AGX_REQUIRE(cfg->tss_max_positions >= 1 && cfg->tss_max_positions <= 1000, AGX_ERR_UNSUPPORTED, "agx_engine_create: tss_max_positions must be in [1, 1000]");
	AGX_REQUIRE(cfg->init_to >= 0 && cfg->init_to <= 3, AGX_ERR_INVALID, "agx_engine_create: init_to must be 0..3");
	AGX_REQUIRE(cfg->solver_yield_fraction >= 0.0f && cfg->solver_yield_fraction <= 1.0f, AGX_ERR_INVALID, "agx_engine_create: solver_yield_fraction must be in [0, 1]");
	AGX_REQUIRE(cfg->final_selector >= 0 && cfg->final_selector <= 5, AGX_ERR_INVALID, "agx_engine_create: final_selector must be 0..5");
	AGX_REQUIRE(cfg->noise_type >= 0 && cfg->noise_type <= 3, AGX_ERR_INVALID, "agx_engine_create: noise_type must be 0 (none), 1 (custom), 2 (dirichlet) or 3 (gumbel)");
	AGX_REQUIRE(cfg->policy_temperature >= 0.0f, AGX_ERR_INVALID, "agx_engine_create: policy_temperature must not be negative");
	AGX_REQUIRE(!cfg->match_mode || cfg->n_games % 2 == 0, AGX_ERR_INVALID, "agx_engine_create: match_mode pairs the trees, n_games must be even");
	AGX_REQUIRE(cfg->noise_weight >= 0.0f && cfg->noise_weight <= 1.0f, AGX_ERR_INVALID, "agx_engine_create: noise_weight must be in [0, 1]");
	AGX_REQUIRE(cfg->search_buffers >= 0 && cfg->search_buffers <= 2, AGX_ERR_INVALID, "agx_engine_create: search_buffers must be 0, 1 or 2");
	{
		const int threads = std::max(1, cfg->search_threads), buffers = (cfg->search_buffers == 2) ? 2 : 1;
		AGX_REQUIRE((threads == 1 && buffers == 1) || (threads * buffers == cfg->n_games && !cfg->match_mode && cfg->solver_yield_fraction == 0.0f), AGX_ERR_INVALID,
				"agx_engine_create: search_threads > 1 / search_buffers = 2 make the pool ONE tree searched by n_games task buffers: n_games must equal "
				"search_threads x buffers (%d x %d), no match_mode, no yielding", threads, buffers);
	}
	AGX_REQUIRE(cfg->record_format >= 0 && cfg->record_format <= 3, AGX_ERR_INVALID, "agx_engine_create: record_format must be 0..3 (bit 0 edge snapshots, bit 1 format-201 samples)");

	AgxEngine *e = new AgxEngine();
	e->cfg = *cfg;
	e->mem.sizing_only = sizing_cus > 0;
	if (const char *fuse = std::getenv("AGX_FUSE_SELECT"))
		e->fuse_select = std::atoi(fuse) != 0;
	EngineDev &d = e->dev;
	std::memset(&d, 0, sizeof(d));
	d.rules = cfg->rules;
	d.n = cfg->board_size;
	d.hw = d.n * d.n;
	d.draw_after = (cfg->draw_after > 0) ? cfg->draw_after : d.hw;
	d.n_games = cfg->n_games;
	d.batch = cfg->max_batch_size;
	d.max_sims = cfg->max_simulations;
	d.c_puct = cfg->exploration_constant;
	d.c_scale = cfg->exploration_scaling;
	d.init_to = cfg->init_to;
	d.leak_threshold = cfg->information_leak_threshold;
	d.expansion_threshold = cfg->policy_expansion_threshold;
	d.max_children = (cfg->max_children > 0) ? cfg->max_children : 0x7FFFFFFF;
	d.tss_max_nodes = cfg->tss_max_positions;
	d.tss_max_depth = 100;
	d.solve_time_ticks = 0ull;
	d.batch_limit = d.batch;
	d.yield_fraction = cfg->solver_yield_fraction;
	d.final_selector = cfg->final_selector;
	d.use_symmetries = cfg->use_symmetries;
	d.symmetry_seed = cfg->symmetry_seed;
	d.noise_type = (cfg->noise_weight > 0.0f) ? cfg->noise_type : 0;
	d.noise_weight = cfg->noise_weight;
	d.noise_seed = cfg->noise_seed;
	const size_t buckets = round_pow2(std::max<size_t>(cfg->tss_table_entries, 4)) / 4;
	d.tt_bucket_mask = buckets - 1;
	d.zobrist_seed = cfg->zobrist_seed;
	d.node_cap = cfg->node_capacity > 0 ? cfg->node_capacity : 8192;
	d.edge_cap = cfg->edge_capacity > 0 ? cfg->edge_capacity : 524288;
	d.edge_cap += d.edge_cap & 1; // even: every arena region then starts on a 16-byte boundary (k_arena_copy moves edges as 16-byte words)
	d.ht_cap = static_cast<int>(round_pow2(4 * static_cast<size_t>(d.node_cap)));
	d.act_cap = d.hw * (d.hw + 1) / 2 + 64;
	d.record_cap = cfg->record_capacity > 0 ? cfg->record_capacity : d.n_games * d.hw;
	d.record_edge_cap = cfg->record_edge_capacity > 0 ? cfg->record_edge_capacity : d.record_cap * 64;
	d.record_format = cfg->record_format;
	d.sample_cap = cfg->record_sample_capacity > 0 ? cfg->record_sample_capacity
			: static_cast<int>(std::min<size_t>(static_cast<size_t>(d.record_cap) * (16 + 6 * static_cast<size_t>(d.hw) + 2), 0x7FFFFFF0u)); // every cell an entry
	d.game_end_cap = cfg->game_end_capacity > 0 ? cfg->game_end_capacity : std::max(2 * d.n_games, d.record_cap / 16); // the record pool fills first

	HostTables tables;
	build_host_tables(cfg->rules, tables);
	std::vector<uint64_t> nc_keys(3 + 3 * d.hw);
	uint64_t st = cfg->zobrist_seed ^ 0x5851F42D4C957F2Dull;
	for (auto &k : nc_keys)
		k = splitmix64(st);
	e->zobrist.resize(4 * d.hw);
	st = cfg->zobrist_seed;
	for (auto &k : e->zobrist)
		k = splitmix64(st);

	int status = AGX_OK;
	const size_t G = d.n_games;
#define AGX_TRY(expr) if (status == AGX_OK) status = (expr)
	AGX_TRY(e->mem.alloc(&d.games, G));
	// tree arenas: pool-wide heaps; every game starts with a class-0 bundle (2 x node_cap nodes, 2 x edge_cap edges, ht_cap table slots),
	// the reserve behind them feeds the games that outgrow theirs (k_arena_service)
	const double reserve = (cfg->arena_reserve >= 0.0f) ? cfg->arena_reserve : 1.0;
	const size_t node_total = static_cast<size_t>(static_cast<double>(G * 2 * d.node_cap) * (1.0 + reserve));
	const size_t edge_total = static_cast<size_t>(static_cast<double>(G * 2 * d.edge_cap) * (1.0 + reserve));
	const size_t ht_total = static_cast<size_t>(static_cast<double>(G * d.ht_cap) * (1.0 + reserve));
	AGX_TRY(e->mem.alloc(&d.nodes, node_total));
	AGX_TRY(e->mem.alloc(&d.edges, edge_total));
	AGX_TRY(e->mem.alloc(&d.ht, ht_total));
	AGX_TRY(e->mem.alloc(&d.heap, 1));
	AGX_TRY(e->mem.alloc(&d.free_bundles, static_cast<size_t>(ARENA_CLASSES) * G));
	AGX_TRY(e->mem.alloc(&d.tasks, G * d.batch));
	// speculative solver: its waves solve several leaves of one game at once, so each wave brings its own spill areas (behind the games')
	e->speculative = cfg->speculative_solver != 0 && cfg->tss_max_positions <= 250 && cfg->max_batch_size <= 16;
	if (e->speculative)
	{
		int cus = sizing_cus, device_of_engine = 0;
		if (sizing_cus <= 0)
		{
			(void) hipGetDevice(&device_of_engine);
			(void) hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_of_engine);
		}
		// default: as many waves as the launch's kernel keeps resident (16 per compute unit on 15x15 boards, 10 on 20x20: its LDS state and registers), but
		// no more than one per leaf of a full batch (a one-tree engine has a few dozen leaves per launch)
		const int per_cu = agx_eng::spec_resident_waves_per_cu(cfg->rules, cfg->board_size);
		e->spec_waves = (cfg->speculative_waves > 0) ? cfg->speculative_waves : std::min<long long>(static_cast<long long>(per_cu) * std::max(1, cus), std::max<long long>(64, static_cast<long long>(G) * cfg->max_batch_size));
		e->spec_waves = std::min(e->spec_waves, SPEC_QUEUE_SLACK);
	}
	// (a group's waves take the areas n_games + group * waves + wave with waves = max(1, spec_waves / n_groups): at least one area per possible group)
	// ... and behind the waves' areas one per park buffer (a parked solve keeps its tails there until the next launch takes it up)
	const bool parking = e->speculative && cfg->rules == AGX_RENJU && cfg->solver_yield_fraction > 0.0f && !cfg->match_mode && std::max(1, cfg->search_threads) == 1;
	const size_t areas = G + static_cast<size_t>(std::max(e->spec_waves, 16)) + (parking ? SPEC_PARK_POOL : 0);
	d.park_area0 = static_cast<int>(G) + std::max(e->spec_waves, 16);
	d.spec_on = e->speculative ? 1 : 0;
	d.park_fraction = parking ? SPEC_PARK_FRACTION : 0.0f;
	if (const char *pf = std::getenv("AGX_PARK_FRACTION")) // (developer knob: the sweep behind SPEC_PARK_FRACTION, profiles/r05_search_variants_ab.txt)
		if (parking && std::atof(pf) > 0.0)
			d.park_fraction = std::min(1.0f, static_cast<float>(std::atof(pf))); // (a fraction of the launch's games: (0, 1])
	AGX_TRY(e->mem.alloc(&d.park_slot, G * d.batch));
	AGX_TRY(e->mem.alloc(&d.park_owner, SPEC_PARK_POOL));
	AGX_TRY(e->mem.alloc(&d.parts_done, 2 * G));
	AGX_TRY(e->mem.memset(d.parts_done, 0, 2 * G * sizeof(int)));
	AGX_TRY(e->mem.alloc(&d.park_lds, parking ? static_cast<size_t>(SPEC_PARK_POOL) * SPEC_PARK_WORDS : 1));
	AGX_TRY(e->mem.memset(d.park_slot, 0, G * d.batch * sizeof(int)));
	AGX_TRY(e->mem.memset(d.park_owner, 0, SPEC_PARK_POOL * sizeof(int)));
	AGX_TRY(e->mem.alloc(&d.act, areas * d.act_cap));
	// per area 20 lists x MAXHW entries: list_get / list_set stride by the kernel's compile-time board (SolverSharedT::HW, = MAXHW in the any-size kernels)
	AGX_TRY(e->mem.alloc(&d.list_spill, areas * 20 * static_cast<size_t>(MAXHW)));
	AGX_TRY(e->mem.alloc(&d.frame_spill, areas * MAX_FRAMES));
	AGX_TRY(e->mem.alloc(&d.snap_spill, areas * static_cast<size_t>(d.hw + 2) * 64)); // undo snapshots: 512 bytes per stone on the board and area
	d.spec_group = 0;
	d.spec_waves = e->spec_waves;
	AGX_TRY(e->mem.alloc(&d.spec_watchdog, 16));
	AGX_TRY(e->mem.memset(d.spec_watchdog, 0, 16 * sizeof(int)));
	AGX_TRY(e->mem.alloc(&d.spec_prof, 16));
	AGX_TRY(e->mem.alloc(&d.spec_trace, 4 * (G + static_cast<size_t>(std::max(e->spec_waves, 16))))); // per game, then per wave (profile builds)
	AGX_TRY(e->mem.memset(d.spec_trace, 0, 4 * (G + static_cast<size_t>(std::max(e->spec_waves, 16))) * sizeof(unsigned long long)));
	AGX_TRY(e->mem.memset(d.spec_prof, 0, 16 * sizeof(unsigned long long)));
	AGX_TRY(e->mem.alloc(&d.spec_items, e->speculative ? G * d.batch + 16 * static_cast<size_t>(SPEC_QUEUE_SLACK) : 1));
	AGX_TRY(e->mem.alloc(&d.spec_left, e->speculative ? G : 1));
	AGX_TRY(e->mem.alloc(&d.spec_tasks, e->speculative ? G * d.batch : 1));
	AGX_TRY(e->mem.alloc(&d.spec_overlay, e->speculative ? G * d.batch * (SPEC_OV_CAP * 16) : 1));
	AGX_TRY(e->mem.alloc(&d.tt, G * buckets * 8));
	AGX_TRY(e->mem.upload(&d.t_pattern, tables.pattern));
	AGX_TRY(e->mem.upload(&d.t_ho3, tables.half_open_three));
	AGX_TRY(e->mem.upload(&d.t_threat, tables.threat));
	{ // the solver's form of the same table: cross type | circle type << 4 in one byte (dev_solver.hpp:threat_lookup)
		std::vector<uint8_t> packed(4096);
		for (int i = 0; i < 4096; i++)
			packed[i] = static_cast<uint8_t>((tables.threat[2 * i] & 15u) | ((tables.threat[2 * i + 1] & 15u) << 4));
		AGX_TRY(e->mem.upload(&d.t_threat_packed, packed));
	}
	AGX_TRY(e->mem.upload(&d.t_defense, tables.defense));
	AGX_TRY(e->mem.upload(&d.nc_keys, nc_keys));
	AGX_TRY(e->mem.upload(&d.zob, e->zobrist));
	AGX_TRY(e->mem.alloc(&d.nn_features, G * d.batch * d.hw));
	AGX_TRY(e->mem.alloc(&d.nn_policy, G * d.batch * d.hw));
	AGX_TRY(e->mem.alloc(&d.nn_value, G * d.batch * 3));
	d.has_q = cfg->action_values ? 1 : 0;
	d.match_mode = cfg->match_mode ? 1 : 0;
	d.prune_root = (cfg->match_mode || !cfg->force_expand_root) ? 1 : 0; // UnifiedGenerator(.., forceExpandRoot): true in self-play (GameGenerator.cpp:183-184), false for a Player (Player.cpp:109)
	d.search_buffers = (cfg->search_buffers == 2) ? 2 : 1;
	d.shared_tree = (cfg->search_threads > 1 || d.search_buffers == 2) ? 1 : 0;
	d.tt_mod = (d.search_buffers == 2) ? std::max(1, cfg->search_threads) : static_cast<int>(G);
	d.grp_first = 0;
	d.grp_count = static_cast<int>(G);
	d.policy_temperature = cfg->policy_temperature;
	e->player[0] = e->player[1] = player_of(d);
	AGX_TRY(e->mem.alloc(&d.nn_q, d.has_q ? G * d.batch * d.hw * 2 : 1));
	AGX_TRY(e->mem.alloc(&d.noise, d.noise_type ? G * d.hw : 1));
	AGX_TRY(e->mem.alloc(&d.nn_list, G * d.batch));
	AGX_TRY(e->mem.alloc(&d.counters, N_COUNTERS));
	AGX_TRY(e->mem.alloc(&d.records, static_cast<size_t>(d.record_cap)));
	AGX_TRY(e->mem.alloc(&d.record_edges, (d.record_format & 1) ? static_cast<size_t>(d.record_edge_cap) : 1));
	AGX_TRY(e->mem.alloc(&d.samples, (d.record_format & 2) ? static_cast<size_t>(d.sample_cap) : 4));
	AGX_TRY(e->mem.alloc(&d.game_ends, static_cast<size_t>(d.game_end_cap)));
	if (status == AGX_OK)
	{
		std::vector<GameState> games(G);
		std::memset(static_cast<void*>(games.data()), 0, G * sizeof(GameState));
		for (size_t g = 0; g < G; g++)
		{
			games[g].node_off[0] = (2 * g) * d.node_cap;
			games[g].node_off[1] = (2 * g + 1) * d.node_cap;
			games[g].edge_off[0] = (2 * g) * static_cast<uint64_t>(d.edge_cap);
			games[g].edge_off[1] = (2 * g + 1) * static_cast<uint64_t>(d.edge_cap);
			games[g].ht_off = g * static_cast<uint64_t>(d.ht_cap);
			games[g].node_cap = d.node_cap;
			games[g].edge_cap = d.edge_cap;
			games[g].ht_cap = d.ht_cap;
		}
		ArenaHeap heap;
		std::memset(&heap, 0, sizeof(heap));
		heap.node_cursor = G * 2 * d.node_cap;
		heap.edge_cursor = G * 2 * static_cast<uint64_t>(d.edge_cap);
		heap.ht_cursor = G * static_cast<uint64_t>(d.ht_cap);
		heap.node_total = node_total;
		heap.edge_total = edge_total;
		heap.ht_total = ht_total;
		heap.free_capacity = static_cast<int32_t>(G);
		e->idle_games = games;
		e->idle_heap = heap;
		AGX_TRY(e->mem.copy_in(d.games, games.data(), G * sizeof(GameState)));
		AGX_TRY(e->mem.copy_in(d.heap, &heap, sizeof(heap)));
		AGX_TRY(e->mem.memset(d.counters, 0, N_COUNTERS * sizeof(int)));
		AGX_TRY(e->mem.memset(d.tasks, 0, G * d.batch * sizeof(DTask)));
		if (e->speculative)
		{
			AGX_TRY(e->mem.memset(d.spec_items, 0, (G * d.batch + 16 * static_cast<size_t>(SPEC_QUEUE_SLACK)) * sizeof(int)));
			AGX_TRY(e->mem.memset(d.spec_tasks, 0, G * d.batch * sizeof(SpecTask)));
			AGX_TRY(e->mem.memset(d.spec_left, 0, G * sizeof(int)));
		}
	}
#undef AGX_TRY
	if (status != AGX_OK)
	{
		e->mem.free_all();
		delete e;
		return status;
	}
	*out = e;
	return AGX_OK;
}

int agx_engine_create(const AgxEngineConfig *cfg, AgxEngine **out)
{
	return engine_create(cfg, out, 0);
}

/* What agx_engine_create(cfg) allocates on a device with `compute_units` compute units, without touching one (a launcher sizing its ranks:
 * GeneratorManager.cpp:146-152 starts one generator thread per device; tests of the multi-GPU plan on a box without a GPU) */
int agx_engine_estimate_device_bytes(const AgxEngineConfig *cfg, int compute_units, unsigned long long *bytes)
{
	AGX_REQUIRE(bytes != nullptr && compute_units > 0, AGX_ERR_INVALID, "agx_engine_estimate_device_bytes: invalid argument");
	AgxEngine *e = nullptr;
	const int st = engine_create(cfg, &e, compute_units);
	if (st != AGX_OK)
		return st;
	*bytes = e->mem.device_bytes;
	delete e;
	return AGX_OK;
}

int agx_engine_destroy(AgxEngine *e)
{
	if (e == nullptr)
		return AGX_OK;
	e->mem.free_all();
	for (hipEvent_t ev : e->events)
		(void) hipEventDestroy(ev);
	for (hipEvent_t ev : e->free_events)
		(void) hipEventDestroy(ev);
	if (e->summary_host != nullptr)
		(void) hipHostFree(e->summary_host);
	if (e->match_sum_host != nullptr)
		(void) hipHostFree(e->match_sum_host);
	if (e->pair_head_host != nullptr)
		(void) hipHostFree(e->pair_head_host);
	if (e->query_host != nullptr)
		(void) hipHostFree(e->query_host);
	delete e;
	return AGX_OK;
}

int agx_engine_begin(AgxEngine *e, const uint16_t *h_openings, int n_openings, void *stream)
{
	AGX_REQUIRE(e != nullptr && h_openings != nullptr, AGX_ERR_INVALID, "agx_engine_begin: null argument");
	AGX_REQUIRE(n_openings > 0, AGX_ERR_INVALID, "agx_engine_begin: need at least one opening");
	uint16_t *d_op = nullptr;
	AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_op), static_cast<size_t>(n_openings) * OPENING_CAP * sizeof(uint16_t)));
	e->mem.pointers.push_back(d_op);
	AGX_HIP_CHECK(hipMemcpy(d_op, h_openings, static_cast<size_t>(n_openings) * OPENING_CAP * sizeof(uint16_t), hipMemcpyHostToDevice));
	e->dev.openings = d_op;
	e->dev.n_openings = n_openings;
	int counters[N_COUNTERS] = { 0 };
	counters[1] = e->dev.match_mode ? 0 : (e->dev.shared_tree ? 1 : e->dev.n_games);
	AGX_HIP_CHECK(hipMemcpy(e->dev.counters, counters, sizeof(counters), hipMemcpyHostToDevice));
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (e->pair_log.head != nullptr) // an empty log, zero totals, shadows at "nothing played"
		AGX_HIP_CHECK(hipMemsetAsync(e->pair_log.head, 0, e->pair_log_bytes, s));
	agx_eng::begin(e->dev, s);
	if (e->dev.match_mode)
	{ // the pairs take openings 0 .. n_games/2 - 1 in order, exactly as they will after finished matches
		EngineDev d = e->dev;
		d.g0 = 0;
		agx_eng::assign_openings(d, d.n_games / 2, s);
		agx_eng::match_restart(d, d.n_games / 2, s);
	}
	AGX_HIP_CHECK(hipGetLastError());
	e->begun = true;
	return AGX_OK;
}

int agx_engine_add_openings(AgxEngine *e, const uint16_t *h_openings, int n_openings)
{
	AGX_REQUIRE(e != nullptr && h_openings != nullptr, AGX_ERR_INVALID, "agx_engine_add_openings: null argument");
	AGX_REQUIRE(n_openings > 0, AGX_ERR_INVALID, "agx_engine_add_openings: need at least one opening");
	AGX_REQUIRE(e->begun, AGX_ERR_STATE, "agx_engine_add_openings: agx_engine_begin has not been called");
	AGX_HIP_CHECK(hipDeviceSynchronize());
	const size_t words_old = static_cast<size_t>(e->dev.n_openings) * OPENING_CAP, words_new = static_cast<size_t>(n_openings) * OPENING_CAP;
	uint16_t *d_op = nullptr;
	AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_op), (words_old + words_new) * sizeof(uint16_t)));
	AGX_HIP_CHECK(hipMemcpy(d_op, e->dev.openings, words_old * sizeof(uint16_t), hipMemcpyDeviceToDevice));
	AGX_HIP_CHECK(hipMemcpy(d_op + words_old, h_openings, words_new * sizeof(uint16_t), hipMemcpyHostToDevice));
	// the previous table is no longer referenced by any launch (device synchronised above): replace it in the allocation list
	for (void *&p : e->mem.pointers)
		if (p == static_cast<const void*>(e->dev.openings))
		{
			(void) hipFree(p);
			p = d_op;
		}
	e->dev.openings = d_op;
	e->dev.n_openings += n_openings;
	return AGX_OK;
}

/* games [first, first + count) of group `group` out of `n_groups` equal parts of the pool */
static int group_range(const AgxEngine *e, int group, int n_groups, EngineDev &d, int &count)
{
	// counters[16 + g] / counters[32 + g] are group g's network count and yield count: at most 16 groups
	AGX_REQUIRE(n_groups >= 1 && n_groups <= 16 && group >= 0 && group < n_groups, AGX_ERR_INVALID, "group %d of %d is not valid (1..16 groups)", group, n_groups);
	const int per = (e->dev.n_games + n_groups - 1) / n_groups;
	d = e->dev;
	d.g0 = group * per;
	count = std::min(per, e->dev.n_games - d.g0);
	d.nn_counter = 16 + group;
	d.yield_counter = 32 + group;
	AGX_REQUIRE(count > 0, AGX_ERR_INVALID, "group %d of %d is empty for %d games", group, n_groups, e->dev.n_games);
	AGX_REQUIRE(!e->dev.shared_tree || n_groups == e->dev.search_buffers, AGX_ERR_INVALID,
			"a tournament-search pool (search_threads) is one tree: it is stepped as a whole, or buffer by buffer (2 groups) when search_buffers = 2 — not in %d groups", n_groups);
	d.grp_first = d.g0;
	d.grp_count = count;
	if (d.match_mode) // a group of a match pool is one player's trees: the launch searches with that player's settings (agx_engine_set_player_search)
		use_player(d, e->player[(d.g0 >= d.n_games / 2) ? 1 : 0]);
	return AGX_OK;
}

} /* extern "C" */

int agx_host::group_stage(AgxEngine *e, const char *name, int group, int n_groups, void *stream, Stage &st)
{
	AGX_REQUIRE(e != nullptr, AGX_ERR_INVALID, "%s: null engine", name);
	AGX_REQUIRE(e->begun, AGX_ERR_STATE, "%s: agx_engine_begin has not been called", name);
	st.s = static_cast<hipStream_t>(stream);
	return group_range(e, group, n_groups, st.d, st.count);
}

/* match mode, both players' trees in one launch per stage: about half of the trees search at any time, so one launch over all of
 * them keeps the GPU as busy as a self-play pool of n_games / 2; only the network stage is split (one slot list per player) */
static int match_stage(AgxEngine *e, void *stream, Stage &st)
{
	AGX_REQUIRE(e != nullptr, AGX_ERR_INVALID, "agx_engine_*_match: null engine");
	AGX_REQUIRE(e->begun, AGX_ERR_STATE, "agx_engine_*_match: agx_engine_begin has not been called");
	AGX_REQUIRE(e->dev.match_mode, AGX_ERR_STATE, "agx_engine_*_match: the engine was not created with match_mode");
	EngineDev &d = st.d;
	d = e->dev;
	d.g0 = 0;
	d.nn_counter = 16;
	d.yield_counter = 32;
	d.match_merged = 1;
	d.player[0] = e->player[0]; // the kernels pick a tree's settings by its half of the pool (dev::use_player_search)
	d.player[1] = e->player[1];
	use_player(d, e->player[0]);
	st.count = d.n_games;
	st.s = static_cast<hipStream_t>(stream);
	return AGX_OK;
}

/* the launches behind an advance kernel that hand larger arenas to the trees that asked for them (a tree's last copy part commits) */
static void service_arenas(const Stage &st, int trees, int assign_count)
{
	agx_eng::arena_service(st.d, trees, assign_count, st.s);
	agx_eng::arena_copy(st.d, trees, st.s);
}

extern "C" {

/* Search::select for every game of the group (Search.cpp:117-158) */
int agx_engine_select_group(AgxEngine *e, int group, int n_groups, void *stream)
{
	Stage st;
	const int status = group_stage(e, "agx_engine_select", group, n_groups, stream, st);
	if (status != AGX_OK)
		return status;
	const EngineDev &d = st.d;
	agx_eng::reset_counter(d.counters + d.nn_counter, d.counters + d.yield_counter, st.s);
	{
		KernelTimer t(e, st.s, 0);
		agx_eng::select(d, d.shared_tree ? 1 : st.count, st.s); // tournament search: one wave walks the threads in turn
	}
	AGX_HIP_CHECK(hipGetLastError());
	return AGX_OK;
}
/* Search::solve + Search::scheduleToNN (Search.cpp:159-199): the threat solver on the selected leaves, then the device-side queue */
int agx_engine_solve_group(AgxEngine *e, int group, int n_groups, void *stream)
{
	Stage st;
	const int status = group_stage(e, "agx_engine_solve", group, n_groups, stream, st);
	if (status != AGX_OK)
		return status;
	{
		KernelTimer t(e, st.s, 1);
		agx_eng::solve(st.d, st.count, false, st.s);
	}
	AGX_HIP_CHECK(hipGetLastError());
	return AGX_OK;
}
/* Search::solve(endTime >= 0) (Search.cpp:159-183, the call of SearchThread::asynchronous_run): node limit `max_nodes` (the reference sets
 * 10 000) and a time budget of `seconds` from the moment the launch starts, shared out task by task like the reference does.  Always the
 * serial solver (one wave per game, straight on the table): overlays of speculative solves hold 256 buckets. */
int agx_engine_solve_timed_group(AgxEngine *e, int group, int n_groups, int max_nodes, double seconds, void *stream)
{
	// (the node limit is looked at once the engine is known to exist and to have begun, and before the group: the order the texts have always come in)
	AGX_REQUIRE(e == nullptr || !e->begun || (max_nodes >= 1 && max_nodes <= 100000), AGX_ERR_INVALID, "agx_engine_solve_timed: node limit %d outside [1, 100000]", max_nodes);
	Stage st;
	const int status = group_stage(e, "agx_engine_solve_timed", group, n_groups, stream, st);
	if (status != AGX_OK)
		return status;
	EngineDev &d = st.d;
	d.tss_max_nodes = max_nodes;
	d.yield_fraction = 0.0f; // every task is solved in this launch: the time limit is what bounds it
	d.solve_time_ticks = (seconds <= 0.0) ? 1ull : static_cast<unsigned long long>(std::min(seconds, 3600.0) * 1.0e8) + 1ull;
	{
		KernelTimer t(e, st.s, 1);
		agx_eng::solve(d, st.count, false, st.s);
	}
	AGX_HIP_CHECK(hipGetLastError());
	return AGX_OK;
}
/* select + solve of the group, in the launch shape the pool was created for */
int agx_engine_select_solve_group(AgxEngine *e, int group, int n_groups, void *stream)
{
	Stage st;
	const int status = group_stage(e, "agx_engine_select", group, n_groups, stream, st);
	if (status != AGX_OK)
		return status;
	EngineDev &d = st.d;
	hipStream_t s = st.s;
	if (e->speculative)
	{ // one persistent launch: games select off a cursor, their leaves are solved in parallel against overlays, committed in batch order
		agx_eng::reset_spec(d.counters + d.nn_counter, nullptr, d.counters + SPEC_COUNTER0 + 4 * group, d.counters + d.yield_counter, s);
		if (d.shared_tree)
		{ // tournament search: the threads descend the one tree in turn (one wave), then their leaves are solved in parallel
			KernelTimer t(e, s, 0);
			agx_eng::select(d, 1, s);
		}
		KernelTimer t(e, s, 1);
		d.spec_group = group;
		d.spec_waves = std::max(1, e->spec_waves / n_groups);
		agx_eng::search_spec(d, st.count, s);
	}
	else if (e->fuse_select && !d.shared_tree)
	{ // one launch: every game selects and solves in its own wave (k_solve<.., FUSED>); timed as the solve stage
		agx_eng::reset_counter(d.counters + d.nn_counter, d.counters + d.yield_counter, s);
		KernelTimer t(e, s, 1);
		agx_eng::solve(d, st.count, true, s);
	}
	else
	{ // two launches: agx_engine_select_group, then agx_engine_solve_group
		agx_eng::reset_counter(d.counters + d.nn_counter, d.counters + d.yield_counter, s);
		{
			KernelTimer t(e, s, 0);
			agx_eng::select(d, d.shared_tree ? 1 : st.count, s);
		}
		KernelTimer t(e, s, 1);
		agx_eng::solve(d, st.count, false, s);
	}
	AGX_HIP_CHECK(hipGetLastError());
	return AGX_OK;
}

int agx_engine_select_solve_match(AgxEngine *e, void *stream)
{
	Stage st;
	const int status = match_stage(e, stream, st);
	if (status != AGX_OK)
		return status;
	EngineDev &d = st.d;
	hipStream_t s = st.s;
	agx_eng::reset_counter(d.counters + 16, d.counters + 32, s);
	agx_eng::reset_counter(d.counters + 17, nullptr, s);
	if (e->speculative)
	{
		agx_eng::reset_spec(d.counters + 16, d.counters + 17, d.counters + SPEC_COUNTER0, d.counters + 32, s);
		KernelTimer t(e, s, 1);
		d.spec_group = 0;
		d.spec_waves = e->spec_waves;
		agx_eng::search_spec(d, d.n_games, s);
	}
	else if (e->fuse_select)
	{
		KernelTimer t(e, s, 1);
		agx_eng::solve(d, d.n_games, true, s);
	}
	else
	{
		{
			KernelTimer t(e, s, 0);
			agx_eng::select(d, d.n_games, s);
		}
		KernelTimer t(e, s, 1);
		agx_eng::solve(d, d.n_games, false, s);
	}
	AGX_HIP_CHECK(hipGetLastError());
	return AGX_OK;
}
int agx_engine_expand_backup_match(AgxEngine *e, void *stream)
{
	Stage st;
	const int status = match_stage(e, stream, st);
	if (status != AGX_OK)
		return status;
	const EngineDev &d = st.d;
	hipStream_t s = st.s;
	{
		KernelTimer t(e, s, 2);
		agx_eng::expand_merged(d, s);
	}
	{
		KernelTimer t(e, s, 3);
		// a moving tree's workgroup also rebases its partner's tree; the partner's own workgroup has nothing to do (it is not searching)
		agx_eng::advance_merged(d, s);
		if (e->pair_log.head != nullptr) // agx_engine_match_track_pairs: the openings this launch finished, in pair order
			agx_eng::match_pair_log(d, e->pair_log, s);
		service_arenas(st, d.n_games, 0);
		agx_eng::assign_openings(d, d.n_games / 2, s);
		agx_eng::clear_tables(d, d.n_games, 0, s);
		agx_eng::match_restart(d, d.n_games / 2, s);
	}
	AGX_HIP_CHECK(hipGetLastError());
	return AGX_OK;
}
int agx_engine_step_match(AgxEngine *e, AgxNet *first_net, AgxNet *second_net, void *stream)
{
	if (e != nullptr && e->dev.match_mode && first_net != nullptr && second_net != nullptr)
	{ // a network without the head a player asks for is refused before anything is launched, not between the two players' forwards
		AgxNet *nets[2] = { first_net, second_net };
		for (int p = 0; p < 2; p++)
		{
			AgxNetDesc desc;
			const int ds = agx_net_description(nets[p], &desc);
			if (ds != AGX_OK)
				return ds;
			AGX_REQUIRE(!e->player[p].has_q || desc.action_values, AGX_ERR_INVALID,
					"agx_engine_step_match: the %s player is configured for a 'pvq' network but its network has no action-values head", p == 0 ? "first" : "second");
		}
	}
	int st = agx_engine_select_solve_match(e, stream);
	if (st == AGX_OK)
		st = agx_engine_evaluate_group(e, first_net, 0, 2, stream);
	if (st == AGX_OK)
		st = agx_engine_evaluate_group(e, second_net, 1, 2, stream);
	if (st == AGX_OK)
		st = agx_engine_expand_backup_match(e, stream);
	return st;
}

int agx_engine_evaluate_group(AgxEngine *e, AgxNet *net, int group, int n_groups, void *stream)
{
	AGX_REQUIRE(e != nullptr && net != nullptr, AGX_ERR_INVALID, "agx_engine_evaluate: null argument");
	EngineDev d;
	int count = 0;
	const int st = group_range(e, group, n_groups, d, count);
	if (st != AGX_OK)
		return st;
	AgxNetDesc desc;
	const int ds = agx_net_description(net, &desc);
	if (ds != AGX_OK)
		return ds;
	// the exchange buffers are laid out with the ENGINE's board (hw cells per slot): a network of another geometry would index them with
	// the wrong stride
	AGX_REQUIRE(desc.rows == d.n && desc.cols == d.n, AGX_ERR_INVALID, "agx_engine_evaluate: the network is built for %dx%d boards, the engine plays on %dx%d",
			desc.rows, desc.cols, d.n, d.n);
	if (d.has_q)
	{
		AGX_REQUIRE(desc.action_values, AGX_ERR_INVALID, "agx_engine_evaluate: the engine was configured for a 'pvq' network but this one has no action-values head");
		return agx_nn_forward_indirect_pvq(net, d.nn_features, d.nn_list + static_cast<size_t>(d.g0) * d.batch, d.counters + d.nn_counter, count * d.batch,
				d.nn_policy, d.nn_value, d.nn_q, stream);
	}
	return agx_nn_forward_indirect(net, d.nn_features, d.nn_list + static_cast<size_t>(d.g0) * d.batch, d.counters + d.nn_counter, count * d.batch, d.nn_policy,
			d.nn_value, stream);
}

} /* extern "C" */

/* Search::generateEdges + expand + backup for every game of the group (Search.cpp:206-232), incl. the move rule's decision */
int agx_host::expand_stage(AgxEngine *e, int group, int n_groups, void *stream, bool with_arena_service)
{
	Stage st;
	const int status = group_stage(e, "agx_engine_expand", group, n_groups, stream, st);
	if (status != AGX_OK)
		return status;
	EngineDev &d = st.d;
	AGX_REQUIRE(!d.match_mode || n_groups == 2, AGX_ERR_INVALID, "agx_engine_expand: a match-mode engine is stepped as two groups (first players, second players)");
	{
		KernelTimer t(e, st.s, 2);
		agx_eng::expand(d, d.shared_tree ? 1 : st.count, st.s);
	}
	if (with_arena_service && e->external_moves && !d.match_mode)
	{ // a caller that makes the moves itself (set_board) never runs the advance stage: the trees that asked for larger arenas get them here
	  // (a pool stepped through expand_group + advance_group — ag::Search::expand, then GameGenerator — has them serviced ONCE, by the advance stage)
		if (d.shared_tree)
			d.g0 = 0;
		service_arenas(st, d.shared_tree ? 1 : st.count, 0);
	}
	AGX_HIP_CHECK(hipGetLastError());
	return AGX_OK;
}

extern "C" {

int agx_engine_expand_group(AgxEngine *e, int group, int n_groups, void *stream)
{
	return expand_stage(e, group, n_groups, stream, true);
}
/* GameGenerator::make_move + prepare_search for the games whose search is complete (GameGenerator.cpp:145-185), then the next openings
 * for the games that ended */
int agx_engine_advance_group(AgxEngine *e, int group, int n_groups, void *stream)
{
	Stage st;
	const int status = group_stage(e, "agx_engine_advance", group, n_groups, stream, st);
	if (status != AGX_OK)
		return status;
	EngineDev &d = st.d;
	hipStream_t s = st.s;
	int count = st.count;
	AGX_REQUIRE(!d.match_mode || n_groups == 2, AGX_ERR_INVALID, "agx_engine_advance: a match-mode engine is stepped as two groups (first players, second players)");
	{
		KernelTimer t(e, s, 3);
		const int trees = d.shared_tree ? 1 : count; // tournament search: one tree (game 0), the other records are its search threads
		if (d.shared_tree)
		{ // (whichever buffer this group is: the tree, its arenas and the restart are record 0's; grp_first / grp_count keep the buffer)
			d.g0 = 0;
			count = d.n_games;
		}
		agx_eng::advance(d, trees, s);
		if (e->pair_log.head != nullptr) // (a match pool that tracks its pairs: either player's move may have ended an opening)
			agx_eng::match_pair_log(d, e->pair_log, s);
		// four launches behind k_advance instead of seven (round 6): the openings are assigned by the service workgroup, a game's last copy part
		// commits its larger arenas, a game's last clear part restarts it
		service_arenas(st, trees, d.match_mode ? 0 : trees);
		if (!d.match_mode)
		{
			agx_eng::clear_tables(d, count, d.shared_tree ? 0 : 1, s);
			if (d.shared_tree)
			{ // the search threads restart on thread 0's opening: they first (they read its request), thread 0 last (it clears the request)
				EngineDev others = d;
				others.g0 = 1;
				if (count > 1)
					agx_eng::restart(others, count - 1, s);
				agx_eng::restart(d, 1, s);
			}
		}
		else if (group == 0)
		{ // restarts go by pair, requested through the first players' trees (= group 0)
			agx_eng::assign_openings(d, count, s);
			{
				EngineDev all = d; // both players' trees
				all.g0 = 0;
				agx_eng::clear_tables(all, all.n_games, 0, s);
			}
			agx_eng::match_restart(d, count, s);
		}
	}
	AGX_HIP_CHECK(hipGetLastError());
	return AGX_OK;
}
int agx_engine_expand_backup_group(AgxEngine *e, int group, int n_groups, void *stream)
{
	const int st = expand_stage(e, group, n_groups, stream, false); // (the advance stage services the arenas)
	return (st != AGX_OK) ? st : agx_engine_advance_group(e, group, n_groups, stream);
}

int agx_engine_step_group(AgxEngine *e, AgxNet *net, int group, int n_groups, void *stream)
{
	int st = agx_engine_select_solve_group(e, group, n_groups, stream);
	if (st == AGX_OK)
		st = agx_engine_evaluate_group(e, net, group, n_groups, stream);
	if (st == AGX_OK)
		st = agx_engine_expand_backup_group(e, group, n_groups, stream);
	return st;
}

int agx_engine_select_solve(AgxEngine *e, void *stream) { return agx_engine_select_solve_group(e, 0, 1, stream); }
int agx_engine_evaluate(AgxEngine *e, AgxNet *net, void *stream) { return agx_engine_evaluate_group(e, net, 0, 1, stream); }
int agx_engine_expand_backup(AgxEngine *e, void *stream) { return agx_engine_expand_backup_group(e, 0, 1, stream); }
int agx_engine_step(AgxEngine *e, AgxNet *net, void *stream) { return agx_engine_step_group(e, net, 0, 1, stream); }

int agx_engine_buffers(AgxEngine *e, AgxEngineBuffers *out)
{
	AGX_REQUIRE(e != nullptr && out != nullptr, AGX_ERR_INVALID, "agx_engine_buffers: null argument");
	out->d_nn_features = e->dev.nn_features;
	out->d_nn_policy = e->dev.nn_policy;
	out->d_nn_value = e->dev.nn_value;
	out->d_nn_action_values = e->dev.has_q ? e->dev.nn_q : nullptr;
	out->d_nn_list = e->dev.nn_list;
	out->d_nn_count = e->dev.counters + 16; /* group 0 of 1 */
	out->slots = e->dev.n_games * e->dev.batch;
	out->cells = e->dev.hw;
	return AGX_OK;
}

int agx_engine_match_results(AgxEngine *e, int *h_results, int pair_capacity)
{
	AGX_REQUIRE(e != nullptr && h_results != nullptr, AGX_ERR_INVALID, "agx_engine_match_results: null argument");
	AGX_REQUIRE(e->dev.match_mode, AGX_ERR_STATE, "agx_engine_match_results: the engine was not created with match_mode");
	const int pairs = e->dev.n_games / 2;
	AGX_REQUIRE(pair_capacity >= pairs, AGX_ERR_INVALID, "agx_engine_match_results: %d pairs do not fit into %d", pairs, pair_capacity);
	AGX_HIP_CHECK(hipDeviceSynchronize());
	std::vector<GameState> games(pairs);
	AGX_HIP_CHECK(hipMemcpy(games.data(), e->dev.games, games.size() * sizeof(GameState), hipMemcpyDeviceToHost));
	for (int i = 0; i < pairs; i++)
	{
		h_results[4 * i + 0] = games[i].match_score[0];
		h_results[4 * i + 1] = games[i].match_score[1];
		h_results[4 * i + 2] = games[i].match_score[2];
		h_results[4 * i + 3] = games[i].games_done;
	}
	return AGX_OK;
}

/* ---- match pools: the pair log (k_match_pair_log) ---- */
int agx_engine_match_track_pairs(AgxEngine *e, int capacity)
{
	AGX_REQUIRE(e != nullptr, AGX_ERR_INVALID, "agx_engine_match_track_pairs: null engine");
	AGX_REQUIRE(e->dev.match_mode, AGX_ERR_STATE, "agx_engine_match_track_pairs: the engine was not created with match_mode");
	AGX_REQUIRE(!e->begun, AGX_ERR_STATE, "agx_engine_match_track_pairs: call it before agx_engine_begin");
	AGX_REQUIRE(capacity >= 1, AGX_ERR_INVALID, "agx_engine_match_track_pairs: capacity %d, need at least 1", capacity);
	AGX_REQUIRE(e->pair_log.head == nullptr, AGX_ERR_STATE, "agx_engine_match_track_pairs: the pool already tracks its pairs (capacity %d)", e->pair_log.capacity);
	const size_t pairs = static_cast<size_t>(e->dev.n_games / 2);
	const size_t bytes = PAIR_LOG_HEAD * sizeof(long long) + pairs * sizeof(int4) + static_cast<size_t>(capacity) * sizeof(AgxPairResult);
	if (e->pair_head_host == nullptr)
		AGX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&e->pair_head_host), PAIR_LOG_HEAD * sizeof(long long), hipHostMallocDefault));
	uint8_t *p = nullptr;
	AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), bytes));
	e->mem.pointers.push_back(p);
	e->mem.device_bytes += bytes;
	AGX_HIP_CHECK(hipMemset(p, 0, bytes));
	e->pair_log.head = reinterpret_cast<long long*>(p);
	e->pair_log.shadow = reinterpret_cast<int4*>(p + PAIR_LOG_HEAD * sizeof(long long));
	e->pair_log.entries = reinterpret_cast<AgxPairResult*>(p + PAIR_LOG_HEAD * sizeof(long long) + pairs * sizeof(int4));
	e->pair_log.capacity = capacity;
	e->pair_log_bytes = bytes;
	return AGX_OK;
}

int agx_engine_match_pair_results(AgxEngine *e, int first, AgxPairResult *h_out, int capacity, long long totals[8], void *stream)
{
	AGX_REQUIRE(e != nullptr && totals != nullptr, AGX_ERR_INVALID, "agx_engine_match_pair_results: null argument");
	AGX_REQUIRE(first >= 0 && capacity >= 0 && (h_out != nullptr || capacity == 0), AGX_ERR_INVALID,
			"agx_engine_match_pair_results: first %d, capacity %d%s", first, capacity, h_out == nullptr ? " with a null buffer" : "");
	AGX_REQUIRE(e->dev.match_mode, AGX_ERR_STATE, "agx_engine_match_pair_results: the engine was not created with match_mode");
	AGX_REQUIRE(e->pair_log.head != nullptr, AGX_ERR_STATE, "agx_engine_match_pair_results: the pool does not track its pairs (agx_engine_match_track_pairs)");
	AGX_REQUIRE(e->begun, AGX_ERR_STATE, "agx_engine_match_pair_results: agx_engine_begin has not been called");
	hipStream_t s = static_cast<hipStream_t>(stream);
	AGX_HIP_CHECK(hipMemcpyAsync(e->pair_head_host, e->pair_log.head, 9 * sizeof(long long), hipMemcpyDeviceToHost, s));
	AGX_HIP_CHECK(hipStreamSynchronize(s));
	std::memcpy(totals, e->pair_head_host, 8 * sizeof(long long));
	const long long logged = e->pair_head_host[8]; // (<= the log's capacity: the kernel's cursor)
	const long long end = std::min(logged, static_cast<long long>(first) + capacity);
	if (end > first)
	{ // the entries are final once written: a later launch only appends
		AGX_HIP_CHECK(hipMemcpyAsync(h_out, e->pair_log.entries + first, static_cast<size_t>(end - first) * sizeof(AgxPairResult), hipMemcpyDeviceToHost, s));
		AGX_HIP_CHECK(hipStreamSynchronize(s));
	}
	return AGX_OK;
}

int agx_engine_set_board(AgxEngine *e, int game, const uint8_t *h_board, int sign_to_move, void *stream)
{
	return agx_engine_set_board_ex(e, game, h_board, sign_to_move, 0, stream);
}
int agx_engine_set_board_ex(AgxEngine *e, int game, const uint8_t *h_board, int sign_to_move, int force_remove_root, void *stream)
{
	AGX_REQUIRE(e != nullptr && h_board != nullptr, AGX_ERR_INVALID, "agx_engine_set_board: null argument");
	AGX_REQUIRE(e->begun, AGX_ERR_STATE, "agx_engine_set_board: agx_engine_begin has not been called");
	AGX_REQUIRE(game >= 0 && game < e->dev.n_games, AGX_ERR_INVALID, "agx_engine_set_board: game %d of %d", game, e->dev.n_games);
	AGX_REQUIRE(sign_to_move == 1 || sign_to_move == 2, AGX_ERR_INVALID, "agx_engine_set_board: sign_to_move must be 1 (cross) or 2 (circle)");
	AGX_REQUIRE(!e->dev.match_mode, AGX_ERR_STATE, "agx_engine_set_board: a match-mode engine plays its own games");
	AGX_REQUIRE(!e->dev.shared_tree || game == 0, AGX_ERR_INVALID, "agx_engine_set_board: a tournament-search engine has one tree, game 0 (records 1.. are its task buffers)");
	for (int i = 0; i < e->dev.hw; i++)
		AGX_REQUIRE(h_board[i] <= 2, AGX_ERR_INVALID, "agx_engine_set_board: cell %d holds %d (0 empty, 1 cross, 2 circle)", i, h_board[i]);
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (e->board_staging == nullptr)
	{
		AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e->board_staging), MAXHW));
		e->mem.pointers.push_back(e->board_staging);
	}
	AGX_HIP_CHECK(hipStreamSynchronize(s)); // (the staging buffer of the previous call may still be read)
	AGX_HIP_CHECK(hipMemcpy(e->board_staging, h_board, e->dev.hw, hipMemcpyHostToDevice));
	{ // Player::setBoard begins with search.cleanup(tree) (Player.cpp:98-100): leaves still in flight give their virtual losses back first
		EngineDev one = e->dev;
		one.g0 = game;
		agx_eng::cancel_pending(one, 1, s);
	}
	agx_eng::set_board(e->dev, game, e->board_staging, sign_to_move, force_remove_root ? 1 : 0, s);
	e->external_moves = true;
	AGX_HIP_CHECK(hipGetLastError());
	return AGX_OK;
}
/* GeneratorThread::saveGames / loadGames (GeneratorManager.cpp:98-122) on the device pool: the games in flight as their move lists */
int agx_engine_save_games(AgxEngine *e, AgxSavedGame *h_out, int capacity, int *count)
{
	AGX_REQUIRE(e != nullptr && count != nullptr, AGX_ERR_INVALID, "agx_engine_save_games: null argument");
	AGX_REQUIRE(e->begun, AGX_ERR_STATE, "agx_engine_save_games: agx_engine_begin has not been called");
	AGX_REQUIRE(!e->dev.match_mode && !e->dev.shared_tree, AGX_ERR_UNSUPPORTED, "agx_engine_save_games: self-play pools only");
	AGX_HIP_CHECK(hipDeviceSynchronize());
	std::vector<GameState> games(e->dev.n_games);
	AGX_HIP_CHECK(hipMemcpy(games.data(), e->dev.games, games.size() * sizeof(GameState), hipMemcpyDeviceToHost));
	int n = 0;
	for (size_t g = 0; g < games.size(); g++)
	{
		const GameState &gs = games[g];
		if (!gs.active || gs.outcome != 0 || gs.error != 0)
			continue; // waiting for an opening, finished (its record is already in the pools) or stopped
		if (h_out != nullptr)
		{
			AGX_REQUIRE(n < capacity, AGX_ERR_INVALID, "agx_engine_save_games: more than %d games in flight", capacity);
			AgxSavedGame &o = h_out[n];
			std::memset(&o, 0, sizeof(o));
			o.game_slot = static_cast<int>(g);
			o.game_index = gs.games_done;
			o.opening_id = gs.opening_id;
			o.sign_to_move = gs.sign_to_move;
			o.nn_queued = gs.nn_queued;
			o.n_moves = gs.n_moves;
			for (int i = 0; i < gs.n_moves; i++)
				o.moves[i] = gs.moves[i];
		}
		n++;
	}
	*count = n;
	return AGX_OK;
}
int agx_engine_restore_game(AgxEngine *e, const AgxSavedGame *game, void *stream)
{
	AGX_REQUIRE(e != nullptr && game != nullptr, AGX_ERR_INVALID, "agx_engine_restore_game: null argument");
	AGX_REQUIRE(e->begun, AGX_ERR_STATE, "agx_engine_restore_game: agx_engine_begin has not been called");
	AGX_REQUIRE(!e->dev.match_mode && !e->dev.shared_tree, AGX_ERR_UNSUPPORTED, "agx_engine_restore_game: self-play pools only");
	AGX_REQUIRE(game->game_slot >= 0 && game->game_slot < e->dev.n_games, AGX_ERR_INVALID, "agx_engine_restore_game: slot %d of %d", game->game_slot, e->dev.n_games);
	AGX_REQUIRE(game->n_moves >= 0 && game->n_moves < e->dev.hw, AGX_ERR_INVALID, "agx_engine_restore_game: %d moves on a board of %d cells", game->n_moves, e->dev.hw);
	std::vector<uint8_t> seen(e->dev.hw, 0);
	for (int i = 0; i < game->n_moves; i++)
	{
		const uint32_t mv = game->moves[i];
		const int sg = mv & 3, r = (mv >> 2) & 127, c = (mv >> 9) & 127;
		AGX_REQUIRE((sg == 1 || sg == 2) && r < e->dev.n && c < e->dev.n && !seen[r * e->dev.n + c], AGX_ERR_INVALID,
				"agx_engine_restore_game: move %d (0x%x) is not a stone on an empty cell", i, mv);
		seen[r * e->dev.n + c] = 1;
	}
	hipStream_t s = static_cast<hipStream_t>(stream);
	if (e->moves_staging == nullptr)
	{
		AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e->moves_staging), MAXHW * sizeof(uint16_t)));
		e->mem.pointers.push_back(e->moves_staging);
	}
	AGX_HIP_CHECK(hipStreamSynchronize(s)); // (the staging buffer of the previous call may still be read)
	AGX_HIP_CHECK(hipMemcpy(e->moves_staging, game->moves, sizeof(uint16_t) * std::max(1, game->n_moves), hipMemcpyHostToDevice));
	agx_eng::restore_game(e->dev, game->game_slot, e->moves_staging, game->n_moves, game->opening_id, game->nn_queued, s);
	AGX_HIP_CHECK(hipGetLastError());
	return AGX_OK;
}
int agx_engine_set_batch_size(AgxEngine *e, int batch_size)
{ // Search::setBatchSize (Search.cpp:252-255): the task buffers keep their capacity (max_batch_size), the select stage fills `batch_size` of it
	AGX_REQUIRE(e != nullptr, AGX_ERR_INVALID, "agx_engine_set_batch_size: null engine");
	AGX_REQUIRE(batch_size >= 1 && batch_size <= e->dev.batch, AGX_ERR_INVALID, "agx_engine_set_batch_size: %d outside [1, max_batch_size = %d]", batch_size, e->dev.batch);
	e->dev.batch_limit = batch_size;
	e->player[0].batch_limit = e->player[1].batch_limit = batch_size; // (a match pool: both players, as before; agx_engine_set_player_search sets one)
	return AGX_OK;
}
int agx_engine_root_summary(AgxEngine *e, int game, void *stream, int *out4)
{
	AGX_REQUIRE(e != nullptr && out4 != nullptr, AGX_ERR_INVALID, "agx_engine_root_summary: null argument");
	AGX_REQUIRE(e->begun, AGX_ERR_STATE, "agx_engine_root_summary: agx_engine_begin has not been called");
	AGX_REQUIRE(game >= 0 && game < e->dev.n_games, AGX_ERR_INVALID, "agx_engine_root_summary: game %d of %d", game, e->dev.n_games);
	if (e->summary_dev == nullptr)
	{
		AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e->summary_dev), 4 * sizeof(int)));
		e->mem.pointers.push_back(e->summary_dev);
		AGX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&e->summary_host), 4 * sizeof(int), hipHostMallocDefault));
	}
	hipStream_t s = static_cast<hipStream_t>(stream);
	EngineDev d = e->dev;
	{ // (k_root_summary reads the game's arenas through its own record)
		agx_eng::root_summary(d, game, e->summary_dev, s);
	}
	AGX_HIP_CHECK(hipMemcpyAsync(e->summary_host, e->summary_dev, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
	AGX_HIP_CHECK(hipStreamSynchronize(s)); // THIS stream only: a network launch on another stream keeps running
	std::memcpy(out4, e->summary_host, 4 * sizeof(int));
	return AGX_OK;
}
namespace
{
	size_t align16(size_t bytes)
	{
		return (bytes + 15) & ~static_cast<size_t>(15);
	}
	/* the query staging buffers hold at least `bytes` (device and pinned host, same size); their previous contents are not kept */
	int query_reserve(AgxEngine *e, size_t bytes)
	{
		if (bytes <= e->query_bytes)
			return AGX_OK;
		const size_t want = std::max(bytes, 2 * e->query_bytes);
		if (e->query_dev != nullptr)
		{
			e->mem.pointers.erase(std::find(e->mem.pointers.begin(), e->mem.pointers.end(), static_cast<void*>(e->query_dev)));
			AGX_HIP_CHECK(hipFree(e->query_dev));
			AGX_HIP_CHECK(hipHostFree(e->query_host));
			e->query_dev = e->query_host = nullptr;
			e->query_bytes = 0;
		}
		AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e->query_dev), want));
		e->mem.pointers.push_back(e->query_dev);
		AGX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&e->query_host), want, hipHostMallocDefault));
		e->query_bytes = want;
		return AGX_OK;
	}
	/* the tree a query reads: the pool slot (match mode: that player's tree), game 0 of a tournament-search engine */
	int query_tree(AgxEngine *e, int game, const char *who)
	{
		AGX_REQUIRE(e->begun, AGX_ERR_STATE, "%s: agx_engine_begin has not been called", who);
		AGX_REQUIRE(game >= 0 && game < e->dev.n_games, AGX_ERR_INVALID, "%s: game %d of %d", who, game, e->dev.n_games);
		AGX_REQUIRE(!e->dev.shared_tree || game == 0, AGX_ERR_INVALID, "%s: a tournament-search engine has one tree, game 0 (records 1.. are its task buffers)", who);
		return AGX_OK;
	}
	int query_moves_on_board(const AgxEngine *e, const uint16_t *moves, int count, const char *who)
	{
		for (int i = 0; i < count; i++)
		{
			const int r = (moves[i] >> 2) & 127, c = (moves[i] >> 9) & 127;
			AGX_REQUIRE(r < e->dev.n && c < e->dev.n, AGX_ERR_INVALID, "%s: move %d (0x%x) is at row %d, column %d of a %dx%d board", who, i, moves[i], r, c, e->dev.n,
					e->dev.n);
		}
		return AGX_OK;
	}
}
int agx_engine_node_info(AgxEngine *e, int game, const uint16_t *h_moves, const int *h_path_offsets, int n_paths, AgxNodeView *h_nodes, AgxEdgeView *h_edges,
		int edges_per_path, void *stream)
{
	AGX_REQUIRE(e != nullptr && h_path_offsets != nullptr && h_nodes != nullptr, AGX_ERR_INVALID, "agx_engine_node_info: null argument");
	AGX_REQUIRE(n_paths >= 0 && edges_per_path >= 0, AGX_ERR_INVALID, "agx_engine_node_info: %d paths, %d edges per path", n_paths, edges_per_path);
	AGX_REQUIRE(edges_per_path == 0 || h_edges != nullptr, AGX_ERR_INVALID, "agx_engine_node_info: h_edges is null but edges_per_path is %d", edges_per_path);
	int status = query_tree(e, game, "agx_engine_node_info");
	if (status != AGX_OK)
		return status;
	AGX_REQUIRE(h_path_offsets[0] == 0, AGX_ERR_INVALID, "agx_engine_node_info: the first path offset is %d, not 0", h_path_offsets[0]);
	for (int i = 0; i < n_paths; i++)
		AGX_REQUIRE(h_path_offsets[i + 1] >= h_path_offsets[i], AGX_ERR_INVALID, "agx_engine_node_info: path %d ends (%d) before it starts (%d)", i,
				h_path_offsets[i + 1], h_path_offsets[i]);
	const int n_moves = h_path_offsets[n_paths];
	AGX_REQUIRE(n_moves == 0 || h_moves != nullptr, AGX_ERR_INVALID, "agx_engine_node_info: h_moves is null");
	if ((status = query_moves_on_board(e, h_moves, n_moves, "agx_engine_node_info")) != AGX_OK)
		return status;
	if (n_paths == 0)
		return AGX_OK;
	// staging: [offsets | moves] in, [nodes | edges] out
	const size_t off_bytes = align16(sizeof(int) * (n_paths + 1)), move_bytes = align16(sizeof(uint16_t) * std::max(1, n_moves));
	const size_t node_bytes = align16(sizeof(AgxNodeView) * n_paths), edge_bytes = sizeof(AgxEdgeView) * static_cast<size_t>(n_paths) * edges_per_path;
	const size_t in_bytes = off_bytes + move_bytes;
	hipStream_t s = static_cast<hipStream_t>(stream); // (the staging buffers are free: every query waits for its own copy back before it returns)
	if ((status = query_reserve(e, in_bytes + node_bytes + edge_bytes)) != AGX_OK)
		return status;
	std::memcpy(e->query_host, h_path_offsets, sizeof(int) * (n_paths + 1));
	if (n_moves > 0)
		std::memcpy(e->query_host + off_bytes, h_moves, sizeof(uint16_t) * n_moves);
	AGX_HIP_CHECK(hipMemcpyAsync(e->query_dev, e->query_host, in_bytes, hipMemcpyHostToDevice, s));
	const int *d_offsets = reinterpret_cast<const int*>(e->query_dev);
	const uint16_t *d_moves = reinterpret_cast<const uint16_t*>(e->query_dev + off_bytes);
	AgxNodeView *d_nodes = reinterpret_cast<AgxNodeView*>(e->query_dev + in_bytes);
	AgxEdgeView *d_edges = reinterpret_cast<AgxEdgeView*>(e->query_dev + in_bytes + node_bytes);
	const int tree = e->dev.shared_tree ? 0 : game;
	agx_eng::node_info(e->dev, n_paths, tree, d_moves, d_offsets, d_nodes, d_edges, edges_per_path, s);
	AGX_HIP_CHECK(hipGetLastError());
	AGX_HIP_CHECK(hipMemcpyAsync(e->query_host + in_bytes, e->query_dev + in_bytes, node_bytes + edge_bytes, hipMemcpyDeviceToHost, s));
	AGX_HIP_CHECK(hipStreamSynchronize(s)); // THIS stream only
	std::memcpy(h_nodes, e->query_host + in_bytes, sizeof(AgxNodeView) * n_paths);
	if (edge_bytes > 0)
		std::memcpy(h_edges, e->query_host + in_bytes + node_bytes, edge_bytes);
	return AGX_OK;
}
int agx_engine_principal_variation(AgxEngine *e, int game, const uint16_t *h_moves, int n_moves, int max_length, uint16_t *h_pv, AgxEdgeView *h_pv_edges,
		AgxNodeView *h_pv_nodes, int *length, void *stream)
{
	AGX_REQUIRE(e != nullptr && length != nullptr && (h_pv != nullptr || max_length == 0), AGX_ERR_INVALID, "agx_engine_principal_variation: null argument");
	AGX_REQUIRE(n_moves >= 0 && (n_moves == 0 || h_moves != nullptr), AGX_ERR_INVALID, "agx_engine_principal_variation: %d moves", n_moves);
	AGX_REQUIRE(max_length >= 0, AGX_ERR_INVALID, "agx_engine_principal_variation: max_length %d", max_length);
	int status = query_tree(e, game, "agx_engine_principal_variation");
	if (status != AGX_OK)
		return status;
	if ((status = query_moves_on_board(e, h_moves, n_moves, "agx_engine_principal_variation")) != AGX_OK)
		return status;
	const int cap = std::min(max_length, e->dev.hw); // (a variation cannot be longer than the board has cells)
	// staging: [moves] in, [length | nodes | edges | pv] out
	const size_t in_bytes = align16(sizeof(uint16_t) * std::max(1, n_moves)), len_bytes = 16;
	const size_t node_bytes = align16(sizeof(AgxNodeView) * (cap + 1)), edge_bytes = align16(sizeof(AgxEdgeView) * std::max(1, cap));
	const size_t pv_bytes = sizeof(uint16_t) * std::max(1, cap), out_bytes = len_bytes + node_bytes + edge_bytes + pv_bytes;
	hipStream_t s = static_cast<hipStream_t>(stream);
	if ((status = query_reserve(e, in_bytes + out_bytes)) != AGX_OK)
		return status;
	if (n_moves > 0)
		std::memcpy(e->query_host, h_moves, sizeof(uint16_t) * n_moves);
	AGX_HIP_CHECK(hipMemcpyAsync(e->query_dev, e->query_host, in_bytes, hipMemcpyHostToDevice, s));
	uint8_t *out_dev = e->query_dev + in_bytes, *out_host = e->query_host + in_bytes;
	const int tree = e->dev.shared_tree ? 0 : game;
	agx_eng::principal_variation(e->dev, tree, reinterpret_cast<const uint16_t*>(e->query_dev), n_moves, cap,
			reinterpret_cast<int*>(out_dev), reinterpret_cast<uint16_t*>(out_dev + len_bytes + node_bytes + edge_bytes),
			reinterpret_cast<AgxEdgeView*>(out_dev + len_bytes + node_bytes), reinterpret_cast<AgxNodeView*>(out_dev + len_bytes), s);
	AGX_HIP_CHECK(hipGetLastError());
	AGX_HIP_CHECK(hipMemcpyAsync(out_host, out_dev, out_bytes, hipMemcpyDeviceToHost, s));
	AGX_HIP_CHECK(hipStreamSynchronize(s)); // THIS stream only
	int n = 0;
	std::memcpy(&n, out_host, sizeof(int));
	*length = n;
	if (n > 0)
		std::memcpy(h_pv, out_host + len_bytes + node_bytes + edge_bytes, sizeof(uint16_t) * n);
	if (h_pv_edges != nullptr && n > 0)
		std::memcpy(h_pv_edges, out_host + len_bytes + node_bytes, sizeof(AgxEdgeView) * n);
	if (h_pv_nodes != nullptr)
		std::memcpy(h_pv_nodes, out_host + len_bytes, sizeof(AgxNodeView) * (n + 1));
	return AGX_OK;
}
int agx_engine_cancel_pending(AgxEngine *e, void *stream)
{
	AGX_REQUIRE(e != nullptr, AGX_ERR_INVALID, "agx_engine_cancel_pending: null engine");
	AGX_REQUIRE(e->begun, AGX_ERR_STATE, "agx_engine_cancel_pending: agx_engine_begin has not been called");
	AGX_REQUIRE(!e->dev.match_mode, AGX_ERR_STATE, "agx_engine_cancel_pending: a match-mode engine plays its own games");
	EngineDev d = e->dev;
	d.g0 = 0;
	agx_eng::cancel_pending(d, d.shared_tree ? 1 : d.n_games, static_cast<hipStream_t>(stream));
	AGX_HIP_CHECK(hipGetLastError());
	return AGX_OK;
}
int agx_engine_set_force_expand_root(AgxEngine *e, int force_expand_root)
{
	AGX_REQUIRE(e != nullptr, AGX_ERR_INVALID, "agx_engine_set_force_expand_root: null engine");
	AGX_REQUIRE(!e->dev.match_mode, AGX_ERR_STATE, "agx_engine_set_force_expand_root: a match-mode engine always prunes the root");
	e->dev.prune_root = force_expand_root ? 0 : 1;
	e->cfg.force_expand_root = force_expand_root ? 1 : 0;
	return AGX_OK;
}
int agx_engine_set_max_simulations(AgxEngine *e, int max_simulations)
{
	AGX_REQUIRE(e != nullptr && max_simulations > 0, AGX_ERR_INVALID, "agx_engine_set_max_simulations: invalid argument");
	e->dev.max_sims = max_simulations;
	e->cfg.max_simulations = max_simulations;
	e->player[0].max_sims = e->player[1].max_sims = max_simulations; // (a match pool: both players, as before; agx_engine_set_player_search sets one)
	return AGX_OK;
}

/* ---- match pools: search settings per player (evaluation/Player.cpp:64-81 takes them from the player's own SelfplayConfig) ---- */
int agx_engine_player_search(AgxEngine *e, int player, AgxPlayerSearch *out)
{
	AGX_REQUIRE(e != nullptr && out != nullptr, AGX_ERR_INVALID, "agx_engine_player_search: null argument");
	AGX_REQUIRE(e->dev.match_mode, AGX_ERR_STATE, "agx_engine_player_search: the engine was not created with match_mode");
	AGX_REQUIRE(player == 0 || player == 1, AGX_ERR_INVALID, "agx_engine_player_search: player must be 0 (first) or 1 (second), not %d", player);
	const PlayerSearchDev &p = e->player[player];
	out->max_simulations = p.max_sims;
	out->max_batch_size = p.batch_limit;
	out->exploration_constant = p.c_puct;
	out->exploration_scaling = p.c_scale;
	out->init_to = p.init_to;
	out->information_leak_threshold = p.leak_threshold;
	out->max_children = (p.max_children == 0x7FFFFFFF) ? 0 : p.max_children;
	out->policy_expansion_threshold = p.expansion_threshold;
	out->policy_temperature = p.policy_temperature;
	out->tss_max_positions = p.tss_max_nodes;
	out->final_selector = p.final_selector;
	out->action_values = p.has_q;
	return AGX_OK;
}
int agx_engine_set_player_search(AgxEngine *e, int player, const AgxPlayerSearch *in)
{
	AGX_REQUIRE(e != nullptr && in != nullptr, AGX_ERR_INVALID, "agx_engine_set_player_search: null argument");
	AGX_REQUIRE(e->dev.match_mode, AGX_ERR_STATE, "agx_engine_set_player_search: the engine was not created with match_mode");
	AGX_REQUIRE(player == 0 || player == 1, AGX_ERR_INVALID, "agx_engine_set_player_search: player must be 0 (first) or 1 (second), not %d", player);
	// (max_simulations below 50: the move rule's threshold can exceed what select ever reaches, AgxEngineConfig.max_simulations.  The pool-wide
	// agx_engine_set_max_simulations keeps accepting any positive value, as before; a player left below 50 by it has to be given a
	// max_simulations >= 50 along with whatever else this call changes)
	AGX_REQUIRE(in->max_simulations >= 50, AGX_ERR_INVALID, "agx_engine_set_player_search: max_simulations must be at least 50, not %d", in->max_simulations);
	AGX_REQUIRE(in->max_batch_size >= 1 && in->max_batch_size <= e->dev.batch, AGX_ERR_INVALID, "agx_engine_set_player_search: max_batch_size %d outside [1, max_batch_size = %d]",
			in->max_batch_size, e->dev.batch);
	AGX_REQUIRE(in->init_to >= 0 && in->init_to <= 3, AGX_ERR_INVALID, "agx_engine_set_player_search: init_to must be 0..3");
	AGX_REQUIRE(in->tss_max_positions >= 1 && in->tss_max_positions <= e->dev.tss_max_nodes, AGX_ERR_INVALID,
			"agx_engine_set_player_search: tss_max_positions must be in [1, %d] (the pool's)", e->dev.tss_max_nodes);
	AGX_REQUIRE(in->final_selector >= 0 && in->final_selector <= 5, AGX_ERR_INVALID, "agx_engine_set_player_search: final_selector must be 0..5");
	AGX_REQUIRE(in->policy_temperature >= 0.0f, AGX_ERR_INVALID, "agx_engine_set_player_search: policy_temperature must not be negative");
	AGX_REQUIRE(in->action_values == 0 || in->action_values == 1, AGX_ERR_INVALID, "agx_engine_set_player_search: action_values must be 0 or 1");
	AGX_REQUIRE(in->action_values == 0 || e->dev.has_q, AGX_ERR_INVALID,
			"agx_engine_set_player_search: action_values = 1 needs a pool created with action_values = 1 (it has no action-values exchange buffer)");
	PlayerSearchDev &p = e->player[player];
	p.max_sims = in->max_simulations;
	p.batch_limit = in->max_batch_size;
	p.c_puct = in->exploration_constant;
	p.c_scale = in->exploration_scaling;
	p.init_to = in->init_to;
	p.leak_threshold = in->information_leak_threshold;
	p.max_children = (in->max_children > 0) ? in->max_children : 0x7FFFFFFF;
	p.expansion_threshold = in->policy_expansion_threshold;
	p.policy_temperature = in->policy_temperature;
	p.tss_max_nodes = in->tss_max_positions;
	p.final_selector = in->final_selector;
	p.has_q = in->action_values;
	return AGX_OK;
}
int agx_engine_match_summary(AgxEngine *e, long long out[4], void *stream)
{
	AGX_REQUIRE(e != nullptr && out != nullptr, AGX_ERR_INVALID, "agx_engine_match_summary: null argument");
	AGX_REQUIRE(e->dev.match_mode, AGX_ERR_STATE, "agx_engine_match_summary: the engine was not created with match_mode");
	AGX_REQUIRE(e->begun, AGX_ERR_STATE, "agx_engine_match_summary: agx_engine_begin has not been called");
	if (e->match_sum_dev == nullptr)
	{
		AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&e->match_sum_dev), 4 * sizeof(long long)));
		e->mem.pointers.push_back(e->match_sum_dev);
	}
	if (e->match_sum_host == nullptr) // (on its own: a call whose second allocation failed must not leave the next one a null pointer)
		AGX_HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&e->match_sum_host), 4 * sizeof(long long), hipHostMallocDefault));
	hipStream_t s = static_cast<hipStream_t>(stream);
	agx_eng::match_summary(e->dev, e->match_sum_dev, s);
	AGX_HIP_CHECK(hipGetLastError());
	AGX_HIP_CHECK(hipMemcpyAsync(e->match_sum_host, e->match_sum_dev, 4 * sizeof(long long), hipMemcpyDeviceToHost, s));
	AGX_HIP_CHECK(hipStreamSynchronize(s));
	std::memcpy(out, e->match_sum_host, 4 * sizeof(long long));
	return AGX_OK;
}
int agx_engine_speculative_waves(AgxEngine *e, int *waves)
{
	AGX_REQUIRE(e != nullptr && waves != nullptr, AGX_ERR_INVALID, "agx_engine_speculative_waves: null argument");
	*waves = e->speculative ? e->spec_waves : 0;
	return AGX_OK;
}
int agx_engine_device_bytes(AgxEngine *e, unsigned long long *bytes)
{
	AGX_REQUIRE(e != nullptr && bytes != nullptr, AGX_ERR_INVALID, "agx_engine_device_bytes: null argument");
	*bytes = e->mem.device_bytes;
	return AGX_OK;
}
int agx_engine_stats(AgxEngine *e, AgxEngineStats *out)
{
	AGX_REQUIRE(e != nullptr && out != nullptr, AGX_ERR_INVALID, "agx_engine_stats: null argument");
	std::vector<GameState> games(e->dev.n_games);
	AGX_HIP_CHECK(hipMemcpy(games.data(), e->dev.games, games.size() * sizeof(GameState), hipMemcpyDeviceToHost));
	int counters[16];
	AGX_HIP_CHECK(hipMemcpy(counters, e->dev.counters, sizeof(counters), hipMemcpyDeviceToHost));
	std::memset(out, 0, sizeof(*out));
	for (const GameState &g : games)
	{
		out->evaluated_nodes += g.stats[0];
		out->network_evaluations += g.stats[1];
		out->information_leaks += g.stats[2];
		out->proven_edge_visits += g.stats[3];
		out->wasted_expansions += g.stats[4];
		out->solver_nodes += g.stats[5];
		out->select_levels += g.stats[6];
		out->select_edge_reads += g.stats[7];
		out->moves_played += g.stats[8];
		out->duplicate_selections += g.stats[9];
		out->speculative_solves += g.spec_stats[0];
		out->speculative_reruns += g.spec_stats[1];
		out->speculative_deferrals += g.spec_stats[2];
		out->speculative_parks += static_cast<int>(g.spec_stats[3]);
		out->peak_nodes = std::max<unsigned long long>(out->peak_nodes, g.stats[10]);
		out->peak_edges = std::max<unsigned long long>(out->peak_edges, g.stats[11]);
		out->active_games += g.active ? 1 : 0;
		if (g.error != 0 && out->first_error == 0)
			out->first_error = g.error;
	}
	if (e->speculative)
	{
		int w[16];
		AGX_HIP_CHECK(hipMemcpy(w, e->dev.spec_watchdog, sizeof(w), hipMemcpyDeviceToHost));
		if (w[0] != 0)
			fprintf(stderr, "[k_search_spec watchdog] a wave waited in vain for queue slot %d: head %d, tail %d, games selected %d of %d, select cursor %d\n", w[1], w[2], w[3], w[4],
					w[5], w[6]);
	}
#ifdef AGX_SPEC_PROFILE
	if (getenv("AGX_SPEC_TRACE"))
	{ // per game of the LAST launch: select done, commit begin, commit end (100 MHz ticks), re-runs * 16 + leaves
		std::vector<unsigned long long> tr(4 * games.size());
		AGX_HIP_CHECK(hipMemcpy(tr.data(), e->dev.spec_trace, tr.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
		FILE *f = fopen(getenv("AGX_SPEC_TRACE"), "w");
		if (f != nullptr)
		{
			for (size_t g = 0; g < games.size(); g++)
				fprintf(f, "%llu %llu %llu %llu\n", tr[4 * g], tr[4 * g + 1], tr[4 * g + 2], tr[4 * g + 3]);
			fclose(f);
		}
		// per wave of the last launches (one per group): select phase over, exit, leaves solved, ticks waited for items
		std::vector<unsigned long long> wv(4 * static_cast<size_t>(std::max(e->spec_waves, 16)));
		AGX_HIP_CHECK(hipMemcpy(wv.data(), e->dev.spec_trace + 4 * games.size(), wv.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
		f = fopen((std::string(getenv("AGX_SPEC_TRACE")) + ".waves").c_str(), "w");
		if (f != nullptr)
		{
			for (size_t w = 0; 4 * w < wv.size(); w++)
				fprintf(f, "%llu %llu %llu %llu\n", wv[4 * w], wv[4 * w + 1], wv[4 * w + 2], wv[4 * w + 3]);
			fclose(f);
		}
	}
	{
		unsigned long long p[16];
		AGX_HIP_CHECK(hipMemcpy(p, e->dev.spec_prof, sizeof(p), hipMemcpyDeviceToHost));
		fprintf(stderr, "[k_search_spec profile, wave-ms summed] select phase %.1f (slowest wave, max over launches %.3f ms), waiting for items %.1f, speculative solves %.1f (%llu, %.1f us each), "
				"commits + re-runs %.1f (longest %.3f ms), longest launch %.3f ms\n", p[0] / 1e5, p[1] / 1e5, p[2] / 1e5, p[3] / 1e5, p[6], p[3] / 1e2 / (p[6] ? p[6] : 1), p[4] / 1e5, p[5] / 1e5,
				p[7] / 1e5);
	}
#endif
#ifdef AGX_SOLVER_PROFILE
	{
		unsigned long long p[10] = { 0 };
		for (const GameState &g : games)
		{
			for (int i = 0; i < 6; i++)
				p[i] += g.prof[i];
			p[6] += g.prof[6] & 0xFFFFFFFFull;
			p[7] += g.prof[6] >> 32;
			p[8] += g.prof[7] & 0xFFFFFFFFull;
			p[9] += g.prof[7] >> 32;
		}
		fprintf(stderr, "[solver profile, 100 MHz ticks] solves %llu: set_board+encode %.1f us, frame machine %.1f us, place/remove %.1f us (%.1f per solve, %.2f us each), total %.1f us per solve\n",
				p[5], p[0] / 100.0 / p[5], p[1] / 100.0 / p[5], p[2] / 100.0 / p[5], (double) p[3] / p[5], p[2] / 100.0 / (p[3] ? p[3] : 1), p[4] / 100.0 / p[5]);
		fprintf(stderr, "[frame machine split, us per solve] table seek %.1f, move generation %.1f, ordering %.1f, evaluate+insert %.1f\n",
				p[6] / 100.0 / p[5], p[7] / 100.0 / p[5], p[8] / 100.0 / p[5], p[9] / 100.0 / p[5]);
		unsigned long long dp[24] = { 0 };
		for (const GameState &g : games)
			for (int i = 0; i < 24; i++)
				dp[i] += g.dprof[i];
		const double solves = static_cast<double>(p[5]);
		fprintf(stderr, "[generate(), shader cycles per solve; %.1f calls] win1 %.0f, loss2 %.0f, win3 %.0f, loss4 %.0f, win5 %.0f, loss6 %.0f, half4 %.0f, rest %.0f\n",
				dp[8] / solves, dp[0] / solves, dp[1] / solves, dp[2] / solves, dp[3] / solves, dp[4] / solves, dp[5] / solves, dp[6] / solves, dp[7] / solves);
		fprintf(stderr, "[frame machine, shader cycles per solve; %.1f loop turns, %.1f picks] resume %.0f, pick %.0f, descend %.0f, child-returned %.0f\n",
				dp[21] / solves, dp[22] / solves, dp[15] / solves, dp[16] / solves, dp[17] / solves, dp[20] / solves);
		fprintf(stderr, "[update_around, shader cycles per solve; %.1f calls, %.2f list changes per call] centre %.0f, gather %.0f, lists %.0f\n",
				dp[14] / solves, dp[13] / (dp[14] ? static_cast<double>(dp[14]) : 1.0), dp[10] / solves, dp[11] / solves, dp[12] / solves);
		fprintf(stderr, "[renju, per solve] forbidden bits of the network input %.1f us, mark_forbidden_moves %.0f shader cycles, generator foul tests %.0f shader cycles (%.2f tests)\n",
				dp[23] / 100.0 / solves, dp[9] / solves, dp[18] / solves, dp[19] / solves);
	}
#endif
	{
		ArenaHeap heap;
		AGX_HIP_CHECK(hipMemcpy(&heap, e->dev.heap, sizeof(heap), hipMemcpyDeviceToHost));
		out->arena_grows = heap.grows;
		out->arena_releases = heap.releases;
		out->arena_failures = heap.failures;
		for (const GameState &g : games)
			out->arena_max_class = std::max(out->arena_max_class, g.arena_class);
		out->arena_heap_used = static_cast<float>(static_cast<double>(heap.edge_cursor) / static_cast<double>(heap.edge_total));
	}
	out->games_finished = counters[2];
	out->openings_taken = counters[1];
	out->records_used = counters[3];
	out->record_edges_used = counters[4];
	return AGX_OK;
}

int agx_engine_game_info(AgxEngine *e, int game, AgxGameInfo *info, uint8_t *h_board, AgxEdgeView *h_root_edges, int edge_capacity)
{
	AGX_REQUIRE(e != nullptr && info != nullptr, AGX_ERR_INVALID, "agx_engine_game_info: null argument");
	AGX_REQUIRE(game >= 0 && game < e->dev.n_games, AGX_ERR_INVALID, "agx_engine_game_info: game %d out of range", game);
	AGX_HIP_CHECK(hipDeviceSynchronize());
	GameState gs;
	AGX_HIP_CHECK(hipMemcpy(&gs, e->dev.games + game, sizeof(GameState), hipMemcpyDeviceToHost));
	info->active = gs.active;
	info->sign_to_move = gs.sign_to_move;
	info->n_moves = gs.n_moves;
	info->outcome = gs.outcome;
	info->error = gs.error;
	info->opening_id = gs.opening_id;
	info->games_done = gs.games_done;
	info->n_nodes = gs.n_nodes;
	info->n_edges = gs.n_edges;
	info->grow_pending = gs.grow_pending;
	info->arena_class = gs.arena_class;
	info->root_visits = 0;
	info->root_win = info->root_draw = 0.0f;
	info->root_score = 0;
	info->root_edges = 0;
	info->root_moves_left = 0.0f;
	info->max_depth = gs.max_depth;
	if (h_board != nullptr)
		std::memcpy(h_board, gs.board, e->dev.hw);
	if (gs.root >= 0)
	{
		DNode root;
		const DNode *nodes = e->dev.nodes + gs.node_off[gs.arena];
		AGX_HIP_CHECK(hipMemcpy(&root, nodes + gs.root, sizeof(DNode), hipMemcpyDeviceToHost));
		info->root_visits = root.visits;
		info->root_win = root.win;
		info->root_draw = root.draw;
		info->root_score = root.score;
		info->root_edges = root.n_edges;
		info->root_moves_left = root.moves_left;
		if (h_root_edges != nullptr)
		{
			AGX_REQUIRE(root.n_edges <= edge_capacity, AGX_ERR_INVALID, "agx_engine_game_info: %d root edges do not fit into %d", root.n_edges, edge_capacity);
			std::vector<DEdge> edges(root.n_edges);
			const DEdge *pool = e->dev.edges + gs.edge_off[gs.arena];
			AGX_HIP_CHECK(hipMemcpy(edges.data(), pool + root.edge_begin, edges.size() * sizeof(DEdge), hipMemcpyDeviceToHost));
			for (int i = 0; i < root.n_edges; i++)
			{
				h_root_edges[i].prior = edges[i].prior;
				h_root_edges[i].win = edges[i].win;
				h_root_edges[i].draw = edges[i].draw;
				h_root_edges[i].visits = edges[i].visits;
				h_root_edges[i].move = edges[i].move;
				h_root_edges[i].score = edges[i].score;
				h_root_edges[i].flag_and_virtual_loss = edges[i].flag_vl;
			}
		}
	}
	return AGX_OK;
}

int agx_engine_fetch_records(AgxEngine *e, AgxMoveRecord *h_records, int record_capacity, AgxEdgeView *h_edges, int edge_capacity, uint8_t *h_samples,
		int sample_capacity, AgxGameEnd *h_game_ends, int game_end_capacity, AgxRecordCounts *counts, int drain)
{
	AGX_REQUIRE(e != nullptr && counts != nullptr, AGX_ERR_INVALID, "agx_engine_fetch_records: null argument");
	AGX_HIP_CHECK(hipDeviceSynchronize());
	int counters[16];
	AGX_HIP_CHECK(hipMemcpy(counters, e->dev.counters, sizeof(counters), hipMemcpyDeviceToHost));
	const int nr = std::min(counters[3], e->dev.record_cap), ne = (e->dev.record_format & 1) ? std::min(counters[4], e->dev.record_edge_cap) : 0;
	const int ns = (e->dev.record_format & 2) ? std::min(counters[6], e->dev.sample_cap) : 0, ng = std::min(counters[7], e->dev.game_end_cap);
	counts->records = nr;
	counts->edges = ne;
	counts->sample_bytes = ns;
	counts->game_ends = ng;
	if (h_records != nullptr)
	{
		AGX_REQUIRE(nr <= record_capacity, AGX_ERR_INVALID, "agx_engine_fetch_records: %d records do not fit into %d", nr, record_capacity);
		std::vector<MoveRecordHeader> headers(nr);
		AGX_HIP_CHECK(hipMemcpy(headers.data(), e->dev.records, headers.size() * sizeof(MoveRecordHeader), hipMemcpyDeviceToHost));
		for (int i = 0; i < nr; i++)
		{
			h_records[i].game_serial = headers[i].game_serial;
			h_records[i].move_number = headers[i].move_number;
			h_records[i].move = headers[i].move;
			h_records[i].root_score = headers[i].root_score;
			h_records[i].root_visits = headers[i].root_visits;
			h_records[i].root_win = headers[i].root_win;
			h_records[i].root_draw = headers[i].root_draw;
			h_records[i].root_flags = headers[i].root_flags;
			h_records[i].n_edges = headers[i].n_edges;
			h_records[i].edge_offset = headers[i].edge_offset;
			h_records[i].game_slot = headers[i].game_slot;
			h_records[i].game_index = headers[i].game_index;
			h_records[i].sample_offset = headers[i].sample_offset;
			h_records[i].sample_bytes = headers[i].sample_bytes;
			h_records[i].outcome = headers[i].outcome;
		}
	}
	if (h_edges != nullptr && ne > 0)
	{
		AGX_REQUIRE(ne <= edge_capacity, AGX_ERR_INVALID, "agx_engine_fetch_records: %d edges do not fit into %d", ne, edge_capacity);
		std::vector<DEdge> edges(ne);
		AGX_HIP_CHECK(hipMemcpy(edges.data(), e->dev.record_edges, edges.size() * sizeof(DEdge), hipMemcpyDeviceToHost));
		for (int i = 0; i < ne; i++)
		{
			h_edges[i].prior = edges[i].prior;
			h_edges[i].win = edges[i].win;
			h_edges[i].draw = edges[i].draw;
			h_edges[i].visits = edges[i].visits;
			h_edges[i].move = edges[i].move;
			h_edges[i].score = edges[i].score;
			h_edges[i].flag_and_virtual_loss = edges[i].flag_vl;
			h_edges[i].reserved = 0;
		}
	}
	if (h_samples != nullptr && ns > 0)
	{
		AGX_REQUIRE(ns <= sample_capacity, AGX_ERR_INVALID, "agx_engine_fetch_records: %d sample bytes do not fit into %d", ns, sample_capacity);
		AGX_HIP_CHECK(hipMemcpy(h_samples, e->dev.samples, static_cast<size_t>(ns), hipMemcpyDeviceToHost));
	}
	if (h_game_ends != nullptr && ng > 0)
	{
		AGX_REQUIRE(ng <= game_end_capacity, AGX_ERR_INVALID, "agx_engine_fetch_records: %d finished games do not fit into %d", ng, game_end_capacity);
		std::vector<GameEndRecord> ends(ng);
		AGX_HIP_CHECK(hipMemcpy(ends.data(), e->dev.game_ends, ends.size() * sizeof(GameEndRecord), hipMemcpyDeviceToHost));
		for (int i = 0; i < ng; i++)
		{
			h_game_ends[i].game_serial = ends[i].game_serial;
			h_game_ends[i].game_slot = ends[i].game_slot;
			h_game_ends[i].game_index = ends[i].game_index;
			h_game_ends[i].outcome = ends[i].outcome;
			h_game_ends[i].n_moves = ends[i].n_moves;
			std::memcpy(h_game_ends[i].moves, ends[i].moves, sizeof(ends[i].moves));
		}
	}
	if (drain)
	{ // the device is synchronised: the pools start empty again (game serials / indices keep counting)
		AGX_HIP_CHECK(hipMemset(e->dev.counters + 3, 0, 2 * sizeof(int)));
		AGX_HIP_CHECK(hipMemset(e->dev.counters + 6, 0, 2 * sizeof(int)));
	}
	return AGX_OK;
}

int agx_engine_records(AgxEngine *e, AgxMoveRecord *h_records, int record_capacity, AgxEdgeView *h_edges, int edge_capacity, int *n_records, int *n_edges)
{
	AGX_REQUIRE(e != nullptr && n_records != nullptr && n_edges != nullptr, AGX_ERR_INVALID, "agx_engine_records: null argument");
	AgxRecordCounts counts;
	const bool sizes_only = (h_records == nullptr || h_edges == nullptr);
	const int st = agx_engine_fetch_records(e, sizes_only ? nullptr : h_records, record_capacity, sizes_only ? nullptr : h_edges, edge_capacity, nullptr, 0, nullptr, 0,
			&counts, 0);
	if (st != AGX_OK)
		return st;
	*n_records = counts.records;
	*n_edges = counts.edges;
	return AGX_OK;
}

int agx_engine_drain_records(AgxEngine *e, AgxMoveRecord *h_records, int record_capacity, AgxEdgeView *h_edges, int edge_capacity, int *n_records, int *n_edges)
{
	AGX_REQUIRE(h_records != nullptr && h_edges != nullptr && n_records != nullptr && n_edges != nullptr, AGX_ERR_INVALID,
			"agx_engine_drain_records: null buffer (query the sizes with agx_engine_records)");
	AgxRecordCounts counts;
	const int st = agx_engine_fetch_records(e, h_records, record_capacity, h_edges, edge_capacity, nullptr, 0, nullptr, 0, &counts, 1);
	if (st != AGX_OK)
		return st;
	*n_records = counts.records;
	*n_edges = counts.edges;
	return AGX_OK;
}

int agx_engine_zobrist(AgxEngine *e, uint64_t *h_keys, size_t n_words)
{
	AGX_REQUIRE(e != nullptr && h_keys != nullptr, AGX_ERR_INVALID, "agx_engine_zobrist: null argument");
	AGX_REQUIRE(n_words == e->zobrist.size(), AGX_ERR_INVALID, "agx_engine_zobrist: expected %zu words", e->zobrist.size());
	std::memcpy(h_keys, e->zobrist.data(), n_words * sizeof(uint64_t));
	return AGX_OK;
}
/* ---- test hooks: single stages on caller-supplied positions ---- */
int agx_engine_kernel_timing(AgxEngine *e, int enable, double *ms_out, long long *launches_out)
{
	AGX_REQUIRE(e != nullptr, AGX_ERR_INVALID, "agx_engine_kernel_timing: null engine");
	AGX_HIP_CHECK(hipDeviceSynchronize());
	double ms[4] = { 0.0, 0.0, 0.0, 0.0 };
	long long launches[4] = { 0, 0, 0, 0 };
	for (size_t i = 0; i < e->event_kernel.size(); i++)
	{
		float t = 0.0f;
		AGX_HIP_CHECK(hipEventElapsedTime(&t, e->events[2 * i], e->events[2 * i + 1]));
		ms[e->event_kernel[i]] += t;
		launches[e->event_kernel[i]]++;
		e->free_events.push_back(e->events[2 * i]);
		e->free_events.push_back(e->events[2 * i + 1]);
	}
	e->events.clear();
	e->event_kernel.clear();
	for (int k = 0; k < 4; k++)
	{
		if (ms_out != nullptr)
			ms_out[k] = ms[k];
		if (launches_out != nullptr)
			launches_out[k] = launches[k];
	}
	e->timing = (enable != 0);
	return AGX_OK;
}

int agx_debug_solve(AgxEngine *e, const uint8_t *h_boards, const int *h_signs, int count, uint32_t *h_features, uint16_t *h_moves, uint16_t *h_scores,
		int *h_counts, uint32_t *h_flags, uint16_t *h_result_scores)
{
	AGX_REQUIRE(e != nullptr && h_boards != nullptr && h_signs != nullptr, AGX_ERR_INVALID, "agx_debug_solve: null argument");
	AGX_REQUIRE(count > 0 && count <= e->dev.n_games, AGX_ERR_INVALID, "agx_debug_solve: count must be in [1, n_games]");
	const EngineDev &d = e->dev;
	uint8_t *d_boards = nullptr;
	int *d_signs = nullptr;
	AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_boards), static_cast<size_t>(count) * d.hw));
	AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_signs), count * sizeof(int)));
	AGX_HIP_CHECK(hipMemcpy(d_boards, h_boards, static_cast<size_t>(count) * d.hw, hipMemcpyHostToDevice));
	AGX_HIP_CHECK(hipMemcpy(d_signs, h_signs, count * sizeof(int), hipMemcpyHostToDevice));
	agx_eng::debug_load_tasks(d, d_boards, d_signs, count, nullptr);
	EngineDev dd = d;
	dd.g0 = 0;
	dd.nn_counter = 16;
	dd.yield_fraction = 0.0f;
	agx_eng::reset_counter(dd.counters + dd.nn_counter, nullptr, nullptr);
	agx_eng::solve(dd, count, false, nullptr);
	AGX_HIP_CHECK(hipGetLastError());
	AGX_HIP_CHECK(hipDeviceSynchronize());
	std::vector<DTask> tasks(1);
	for (int g = 0; g < count; g++)
	{
		AGX_HIP_CHECK(hipMemcpy(tasks.data(), d.tasks + static_cast<size_t>(g) * d.batch, sizeof(DTask), hipMemcpyDeviceToHost));
		const DTask &t = tasks[0];
		h_counts[g] = t.n_edges;
		h_flags[g] = t.flags;
		h_result_scores[g] = static_cast<uint16_t>(t.score);
		for (int i = 0; i < t.n_edges; i++)
		{
			h_moves[static_cast<size_t>(g) * d.hw + i] = t.emove[i];
			h_scores[static_cast<size_t>(g) * d.hw + i] = t.escore[i];
		}
		if (h_features != nullptr)
			AGX_HIP_CHECK(hipMemcpy(h_features + static_cast<size_t>(g) * d.hw, d.nn_features + static_cast<size_t>(g) * d.batch * d.hw, d.hw * sizeof(uint32_t),
					hipMemcpyDeviceToHost));
	}
	{ // solver nodes of every position (GameState::stats[5]) for agx_debug_solve_nodes
		std::vector<GameState> after(count);
		AGX_HIP_CHECK(hipMemcpy(after.data(), d.games, static_cast<size_t>(count) * sizeof(GameState), hipMemcpyDeviceToHost));
		e->debug_solve_nodes.resize(count);
		for (int g = 0; g < count; g++)
			e->debug_solve_nodes[g] = after[g].stats[5];
	}
	// leave the pool idle again
	AGX_HIP_CHECK(hipMemcpy(d.games, e->idle_games.data(), e->idle_games.size() * sizeof(GameState), hipMemcpyHostToDevice)); // idle pool, arena descriptors intact
	(void) hipFree(d_boards);
	(void) hipFree(d_signs);
	return AGX_OK;
}

int agx_debug_solve_nodes(AgxEngine *e, int count, unsigned long long *h_nodes)
{
	AGX_REQUIRE(e != nullptr && h_nodes != nullptr, AGX_ERR_INVALID, "agx_debug_solve_nodes: null argument");
	AGX_REQUIRE(count >= 0 && static_cast<size_t>(count) <= e->debug_solve_nodes.size(), AGX_ERR_INVALID, "agx_debug_solve_nodes: the last agx_debug_solve solved %zu positions",
			e->debug_solve_nodes.size());
	for (int g = 0; g < count; g++)
		h_nodes[g] = e->debug_solve_nodes[g];
	return AGX_OK;
}

/*
 * OpeningGenerator::generate (src/selfplay/OpeningGenerator.cpp:21-78), batched: candidates from prepareOpening(config, 1), each
 * given to the threat solver with a 1000-node budget (:61-62) and redrawn (up to 100 times, :55) while the solver proves it; the
 * survivors are evaluated by the network and, in workspace order, accepted when |E - 0.5| < 0.1 + 0.01 * trials (:41-48).
 */
int agx_engine_generate_openings(AgxEngine *e, AgxNet *net, int count, uint32_t seed, uint16_t *h_openings, int *h_stats)
{
	AGX_REQUIRE(e != nullptr && net != nullptr && h_openings != nullptr, AGX_ERR_INVALID, "agx_engine_generate_openings: null argument");
	AGX_REQUIRE(count > 0, AGX_ERR_INVALID, "agx_engine_generate_openings: count must be positive");
	AGX_REQUIRE(!e->begun, AGX_ERR_STATE, "agx_engine_generate_openings: the pool is playing (the generator borrows its task slots); call it before agx_engine_begin");
	const EngineDev &d = e->dev;
	const int W = std::min(d.n_games, 64); // workspace entries evaluated together (the reference uses max_batch_size of them)
	struct Entry
	{
			uint16_t opening[AGX_OPENING_CAP];
			bool scheduled = false;
			float expectation = 0.0f;
	};
	std::vector<Entry> workspace(W);
	std::vector<uint8_t> boards(static_cast<size_t>(W) * d.hw);
	std::vector<int> signs(W), todo;
	std::vector<DTask> task(1);
	std::vector<float> values(static_cast<size_t>(W) * d.batch * 3);
	uint8_t *d_boards = nullptr;
	int *d_signs = nullptr;
	AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_boards), boards.size()));
	AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_signs), W * sizeof(int)));
	EngineDev dd = d;
	dd.g0 = 0;
	dd.nn_counter = 16;
	dd.yield_fraction = 0.0f;
	dd.use_symmetries = 0;
	dd.tss_max_nodes = 1000; // solver.setNodeLimit(1000)
	int completed = 0, trials = 0;
	long long stats[4] = { 0, 0, 0, 0 }; // candidates drawn, proven by the solver, rejected as unbalanced, network evaluations
	int status = AGX_OK;
	while (completed < count && status == AGX_OK)
	{
		for (int attempt = 0; attempt < 100; attempt++)
		{
			todo.clear();
			for (int i = 0; i < W; i++)
				if (!workspace[i].scheduled)
					todo.push_back(i);
			if (todo.empty())
				break;
			const int m = static_cast<int>(todo.size());
			for (int j = 0; j < m; j++)
			{
				Entry &en = workspace[todo[j]];
				if ((status = agx_make_opening(d.rules, d.n, seed++, en.opening)) != AGX_OK)
					break;
				stats[0]++;
				uint8_t *b = boards.data() + static_cast<size_t>(j) * d.hw;
				std::memset(b, 0, d.hw);
				for (int k = 0; k < en.opening[0]; k++)
				{
					const uint16_t mv = en.opening[1 + k];
					b[((mv >> 2) & 127) * d.n + ((mv >> 9) & 127)] = mv & 3;
				}
				signs[j] = (en.opening[0] == 0) ? AGX_CROSS : (3 - (en.opening[en.opening[0]] & 3));
			}
			if (status != AGX_OK)
				break;
			AGX_HIP_CHECK(hipMemcpy(d_boards, boards.data(), static_cast<size_t>(m) * d.hw, hipMemcpyHostToDevice));
			AGX_HIP_CHECK(hipMemcpy(d_signs, signs.data(), m * sizeof(int), hipMemcpyHostToDevice));
			agx_eng::debug_load_tasks(dd, d_boards, d_signs, m, nullptr);
			agx_eng::reset_counter(dd.counters + dd.nn_counter, nullptr, nullptr);
			agx_eng::solve(dd, m, false, nullptr);
			AGX_HIP_CHECK(hipGetLastError());
			// the unproven positions are in the pool's slot list exactly as after a search step: evaluate them
			if ((status = agx_nn_forward_indirect(net, dd.nn_features, dd.nn_list, dd.counters + dd.nn_counter, m * dd.batch, dd.nn_policy, dd.nn_value, nullptr))
					!= AGX_OK)
				break;
			AGX_HIP_CHECK(hipDeviceSynchronize());
			AGX_HIP_CHECK(hipMemcpy(values.data(), dd.nn_value, static_cast<size_t>(m) * dd.batch * 3 * sizeof(float), hipMemcpyDeviceToHost));
			for (int j = 0; j < m; j++)
			{
				AGX_HIP_CHECK(hipMemcpy(task.data(), dd.tasks + static_cast<size_t>(j) * dd.batch, offsetof(DTask, path_node), hipMemcpyDeviceToHost));
				Entry &en = workspace[todo[j]];
				if (task[0].needs_nn)
				{
					const float *v = values.data() + static_cast<size_t>(j) * dd.batch * 3;
					en.expectation = v[0] + 0.5f * v[1];
					en.scheduled = true;
					stats[3]++;
				}
				else
					stats[1]++;
			}
		}
		if (status != AGX_OK)
			break;
		for (int i = 0; i < W && completed < count; i++)
		{
			Entry &en = workspace[i];
			if (!en.scheduled)
				continue; // proven 100 times in a row: the reference leaves such an entry for the next call as well
			const float balance = std::fabs(en.expectation - 0.5f);
			if (balance < (0.1f + 0.01f * trials))
			{
				std::memcpy(h_openings + static_cast<size_t>(completed) * AGX_OPENING_CAP, en.opening, sizeof(en.opening));
				completed++;
				trials = 0;
			}
			else
			{
				trials++;
				stats[2]++;
			}
			en.scheduled = false;
		}
		for (Entry &en : workspace)
			en.scheduled = false; // entries not consumed because enough openings were found
	}
	(void) hipMemcpy(d.games, e->idle_games.data(), e->idle_games.size() * sizeof(GameState), hipMemcpyHostToDevice); // leave the pool idle again
	(void) hipFree(d_boards);
	(void) hipFree(d_signs);
	if (h_stats != nullptr)
		for (int i = 0; i < 4; i++)
			h_stats[i] = static_cast<int>(stats[i]);
	return status;
}

int agx_debug_new_generation(AgxEngine *e)
{ // AlphaBetaSearch::increaseGeneration (AlphaBetaSearch.cpp:63-66) for the positions agx_debug_solve solves: every game's solver table ages by one
	AGX_REQUIRE(e != nullptr, AGX_ERR_INVALID, "agx_debug_new_generation: null engine");
	// (agx_debug_solve leaves the pool idle after every call: the generation lives in the idle template it restores)
	for (GameState &g : e->idle_games)
		g.generation = (g.generation + 1) % 64;
	AGX_HIP_CHECK(hipMemcpy(e->dev.games, e->idle_games.data(), e->idle_games.size() * sizeof(GameState), hipMemcpyHostToDevice));
	return AGX_OK;
}

int agx_debug_pattern_state(AgxEngine *e, const uint8_t *h_boards, const int *h_signs, const uint16_t *h_moves, int count, int n_moves, uint8_t *h_ptypes,
		uint8_t *h_threats, int16_t *h_lists, int lists_stride)
{
	AGX_REQUIRE(e != nullptr, AGX_ERR_INVALID, "agx_debug_pattern_state: null engine");
	AGX_REQUIRE(count > 0 && count <= e->dev.n_games, AGX_ERR_INVALID, "agx_debug_pattern_state: count must be in [1, n_games] (a position uses its game's spill areas)");
	const EngineDev &d = e->dev;
	uint8_t *d_boards = nullptr, *d_pt = nullptr, *d_th = nullptr;
	int *d_signs = nullptr;
	uint16_t *d_moves = nullptr;
	int16_t *d_lists = nullptr;
	const size_t cells = static_cast<size_t>(count) * d.hw;
	AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_boards), cells));
	AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_signs), count * sizeof(int)));
	AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_moves), std::max<size_t>(static_cast<size_t>(count) * n_moves * 2, 16)));
	AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_pt), cells * 8));
	AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_th), cells * 2));
	AGX_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_lists), static_cast<size_t>(count) * lists_stride * 2));
	AGX_HIP_CHECK(hipMemcpy(d_boards, h_boards, cells, hipMemcpyHostToDevice));
	AGX_HIP_CHECK(hipMemcpy(d_signs, h_signs, count * sizeof(int), hipMemcpyHostToDevice));
	if (n_moves > 0)
		AGX_HIP_CHECK(hipMemcpy(d_moves, h_moves, static_cast<size_t>(count) * n_moves * 2, hipMemcpyHostToDevice));
	agx_eng::debug_pattern_state(d, count, d_boards, d_signs, d_moves, n_moves, d_pt, d_th, d_lists, lists_stride, nullptr);
	AGX_HIP_CHECK(hipGetLastError());
	AGX_HIP_CHECK(hipDeviceSynchronize());
	AGX_HIP_CHECK(hipMemcpy(h_ptypes, d_pt, cells * 8, hipMemcpyDeviceToHost));
	AGX_HIP_CHECK(hipMemcpy(h_threats, d_th, cells * 2, hipMemcpyDeviceToHost));
	AGX_HIP_CHECK(hipMemcpy(h_lists, d_lists, static_cast<size_t>(count) * lists_stride * 2, hipMemcpyDeviceToHost));
	(void) hipFree(d_boards);
	(void) hipFree(d_signs);
	(void) hipFree(d_moves);
	(void) hipFree(d_pt);
	(void) hipFree(d_th);
	(void) hipFree(d_lists);
	return AGX_OK;
}

/* host-only: the lookup tables the engine uploads (for CPU-side verification against the reference) */
int agx_host_tables(int rules, uint8_t *h_pattern, uint8_t *h_half_open_three, uint8_t *h_threat, uint16_t *h_defense)
{
	AGX_REQUIRE(rules >= 0 && rules <= AGX_CARO6, AGX_ERR_INVALID, "agx_host_tables: unknown rules %d", rules);
	HostTables t;
	build_host_tables(rules, t);
	if (h_pattern != nullptr)
		std::memcpy(h_pattern, t.pattern.data(), t.pattern.size());
	if (h_half_open_three != nullptr)
		std::memcpy(h_half_open_three, t.half_open_three.data(), t.half_open_three.size());
	if (h_threat != nullptr)
		std::memcpy(h_threat, t.threat.data(), t.threat.size());
	if (h_defense != nullptr)
		std::memcpy(h_defense, t.defense.data(), t.defense.size() * sizeof(uint16_t));
	return AGX_OK;
}

} /* extern "C" */
