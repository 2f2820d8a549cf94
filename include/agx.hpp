/*
 * agx.hpp — C++ host facade over the C ABI (agx.h), mirroring the reference's operator interface for the self-play path.
 *
 * Same names, argument meaning and error behaviour as the reference classes it stands in for:
 *   agx::AGNetwork      <- ag::AGNetwork   (include/alphagomoku/networks/AGNetwork.hpp:60-98): loadWeights / forward / setBatchSize-free
 *   agx::GeneratorPool  <- one ag::GeneratorThread with its GameGenerators (src/selfplay/GeneratorManager.cpp:124-141,
 *                          src/selfplay/GameGenerator.cpp:46-121): generate() = one select/solve/evaluate/expand/backup/move step
 * Errors surface as std::runtime_error / std::logic_error exactly where the reference throws (NNEvaluator.cpp:149,185-187).
 * Header-only convenience layer (used by csrc/selfplay_main.cpp); link with -lagx.  The compiled, reference-NAMED classes — ag::NNEvaluator,
 * ag::Search, ag::Tree, ag::GameGenerator, ag::GeneratorThread, ag::GeneratorManager, ag::GameDataBuffer — live in
 * include/alphagomoku_agx/ (libagx_ag.so).
 */
#ifndef AGX_HPP_
#define AGX_HPP_

#include "agx.h"

#include <algorithm>
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <atomic>
#include <vector>

namespace agx
{
	inline void check(int status)
	{
		if (status == AGX_OK)
			return;
		const std::string msg = agx_last_error();
		if (status == AGX_ERR_INVALID || status == AGX_ERR_STATE)
			throw std::logic_error(msg);
		throw std::runtime_error(msg);
	}

	/* Keeps a launch loop at most `ahead` steps in front of a stream: call step(stream) behind every step's launches.  Without it the host
	 * enqueues until the launch queue is full and spins there — a whole CPU per device thread; with it the thread sleeps on a blocking event
	 * (agx.h: agx_event_create_blocking).  Pacing only: the device never waits for the host while `ahead` >= 1 step is queued. */
	class HostPacer
	{
			std::vector<void*> m_events;
			uint64_t m_count = 0;
			int m_ahead;
		public:
			explicit HostPacer(int ahead = 2) :
					m_events(static_cast<size_t>(ahead > 0 ? ahead + 1 : 0), nullptr), m_ahead(ahead)
			{
				for (void *&e : m_events)
					check(agx_event_create_blocking(&e));
			}
			HostPacer(const HostPacer&) = delete;
			HostPacer& operator=(const HostPacer&) = delete;
			HostPacer(HostPacer &&other) noexcept :
					m_events(std::move(other.m_events)), m_count(other.m_count), m_ahead(other.m_ahead)
			{
				other.m_events.clear();
			}
			~HostPacer()
			{
				for (void *e : m_events)
					agx_event_destroy(e);
			}
			void step(void *stream)
			{
				if (m_ahead <= 0)
					return;
				const size_t ring = m_events.size();
				check(agx_event_record(m_events[m_count % ring], stream));
				if (m_count >= static_cast<uint64_t>(m_ahead))
					check(agx_event_synchronize(m_events[(m_count - m_ahead) % ring]));
				m_count++;
			}
	};

	struct GameConfig
	{ // ag::GameConfig (utils/configs.hpp:23-44)
			int rules = AGX_FREESTYLE;
			int rows = 15, cols = 15;
			int draw_after = 225;
	};

	class AGNetwork
	{
			AgxNet *m_net = nullptr;
			AgxNetDesc m_desc { };
			int m_architecture = AGX_ARCH_RESNET, m_moves_left = 0;
		public:
			/* architecture "ResnetPV" (networks.cpp:71-93), "ResnetPVQ" (:143-168, adds the action-values head), "BottleneckPV" (:170-204),
			 * "BottleneckPVraw" (:206-240, the 8 low bits of a feature word in), "BottleneckPVQ" (:324-361), "ConvNextPVQraw" (:1078-1140) or
			 * "ConvNextPVQMraw" (:1142-1219, adds the moves-left output) */
			AGNetwork(const GameConfig &cfg, int blocks, int filters, const std::string &architecture = "ResnetPV")
			{
				const bool convnext = (architecture == "ConvNextPVQraw" || architecture == "ConvNextPVQMraw");
				const bool bottleneck = (architecture == "BottleneckPV" || architecture == "BottleneckPVraw" || architecture == "BottleneckPVQ");
				if (architecture != "ResnetPV" && architecture != "ResnetPVQ" && !convnext && !bottleneck)
					throw std::logic_error("AGNetwork: unknown architecture '" + architecture + "'");
				m_architecture = convnext ? AGX_ARCH_CONVNEXT : (bottleneck ? AGX_ARCH_BOTTLENECK : AGX_ARCH_RESNET);
				m_moves_left = (architecture == "ConvNextPVQMraw") ? 1 : 0;
				m_desc.action_values = (architecture == "ResnetPVQ" || architecture == "BottleneckPVQ" || convnext) ? 1 : 0;
				m_desc.rows = cfg.rows;
				m_desc.cols = cfg.cols;
				m_desc.blocks = blocks;
				m_desc.filters = filters;
				m_desc.in_channels = (convnext || architecture == "BottleneckPVraw") ? 8 : 32;
				m_desc.value_hidden = convnext ? 256 : ((2 * filters < 256) ? 2 * filters : 256);
				check(agx_net_create_ex(&m_desc, m_architecture, m_moves_left, &m_net));
			}
			AGNetwork(const AGNetwork&) = delete;
			AGNetwork& operator=(const AGNetwork&) = delete;
			~AGNetwork()
			{
				agx_net_destroy(m_net);
			}
			size_t numberOfWeights() const
			{
				return agx_net_blob_floats_ex(&m_desc, m_architecture, m_moves_left);
			}
			void loadWeights(const std::vector<float> &blob)
			{
				check(agx_net_load_weights(m_net, blob.data(), blob.size()));
			}
			/* device buffers: features uint32[batch][rows*cols] -> policy float[batch][rows*cols], value float[batch][3] */
			void forward(const uint32_t *d_features, int batch, float *d_policy, float *d_value, void *stream = nullptr)
			{
				check(agx_nn_forward(m_net, d_features, batch, d_policy, d_value, stream));
			}
			/* 'pvq' networks: additionally action values float[batch][rows*cols][2] = (win, draw) */
			void forward(const uint32_t *d_features, int batch, float *d_policy, float *d_value, float *d_action_values, void *stream)
			{
				check(agx_nn_forward_pvq(m_net, d_features, batch, d_policy, d_value, d_action_values, stream));
			}
			/* 'pvqm' networks: additionally moves left float[batch][rows*cols], the softmax of the 'm' output */
			void forward(const uint32_t *d_features, int batch, float *d_policy, float *d_value, float *d_action_values, float *d_moves_left, void *stream)
			{
				check(agx_nn_forward_pvqm(m_net, d_features, batch, d_policy, d_value, d_action_values, d_moves_left, stream));
			}
			std::string getOutputConfig() const
			{ // AGNetwork::getOutputConfig
				return m_moves_left ? "pvqm" : (m_desc.action_values ? "pvq" : "pv");
			}
			AgxNet* handle() const noexcept
			{
				return m_net;
			}
			const AgxNetDesc& description() const noexcept
			{
				return m_desc;
			}
	};

	struct SearchConfig
	{ // the fields of ag::SearchConfig / MCTSConfig / EdgeSelectorConfig / TreeConfig / TSSConfig that the path reads
			int max_batch_size = 8;
			float exploration_constant = 1.25f;
			float exploration_scaling = 0.0f;
			std::string init_to = "q_head";
			std::string noise_type = "none";      // EdgeSelectorConfig::noise_type: "none", "custom", "dirichlet", "gumbel"
			float noise_weight = 0.0f;
			float policy_expansion_threshold = 1.0e-4f;
			float policy_temperature = 1.0f; // MCTSConfig::policy_temperature
			int max_children = 0;                 // MCTSConfig::max_children, 0 = unlimited
			float information_leak_threshold = 0.01f;
			int tss_max_positions = 100;
			uint64_t tss_table_entries = 4ull * 1024ull * 1024ull;
	};
	inline int final_selector_id(const std::string &policy)
	{ // EdgeSelector::create (EdgeSelector.cpp:680-711): the selectors GameGenerator::make_move can be configured with
		if (policy == "best") return 0;
		if (policy == "max_visit") return 1;
		if (policy == "min_visit") return 2;
		if (policy == "max_value") return 3;
		if (policy == "max_policy") return 4;
		if (policy == "lcb") return 5;
		throw std::logic_error("Unknown selection policy '" + policy + "'");
	}

	struct SelfplayConfig
	{ // ag::SelfplayConfig subset (utils/configs.hpp:205-255)
			int games_per_thread = 1024;
			int max_simulations = 400;
			bool use_symmetries = false;         // SelfplayConfig::use_symmetries -> NNEvaluator::useSymmetries
			std::string network_outputs = "pv";  // AGNetwork::getOutputConfig of the network that will evaluate: "pv" or "pvq"
			std::string final_selector = "best"; // SelfplayConfig::final_selector.policy
			int record_format = 1;               // AgxEngineConfig::record_format: 1 root-edge snapshots, 2 format-201 samples, 3 both
			SearchConfig search_config;
	};

	class GeneratorPool
	{
			AgxEngine *m_engine = nullptr;
			AgxEngineBuffers m_buffers { };
			std::vector<void*> m_slice_streams; // useChipSlices: one CU-masked stream per slice of the pool
			std::vector<HostPacer> m_pacers;    // one per slice (or one for the un-sliced pool)
			int m_steps_ahead = 2;
			int m_pair_capacity = 0; // trackPairs: the pair log's entries
			bool m_phase_started = false, m_skip_first_search_of_slice0 = false;
			int m_games = 0;
			bool m_match = false;
		public:
			/* evaluationMatches: the pool plays EvaluationGames instead (evaluation/EvaluationGame.cpp): games_per_thread pairs of Players,
			 * one tree per Player, every opening twice with the colours swapped; drive it with generate(first, second) */
			GeneratorPool(const GameConfig &game, const SelfplayConfig &selfplay, bool evaluationMatches = false)
			{
				AgxEngineConfig c;
				check(agx_engine_default_config(&c));
				c.rules = game.rules;
				c.board_size = game.rows;
				c.draw_after = game.draw_after;
				c.n_games = evaluationMatches ? 2 * selfplay.games_per_thread : selfplay.games_per_thread;
				c.match_mode = evaluationMatches ? 1 : 0;
				c.max_batch_size = selfplay.search_config.max_batch_size;
				c.max_simulations = selfplay.max_simulations;
				c.exploration_constant = selfplay.search_config.exploration_constant;
				c.exploration_scaling = selfplay.search_config.exploration_scaling;
				const std::string &init = selfplay.search_config.init_to;
				c.init_to = (init == "q_head") ? 0 : (init == "parent") ? 1 : (init == "draw") ? 2 : 3; // EdgeSelector.cpp:1140-1165
				c.policy_expansion_threshold = selfplay.search_config.policy_expansion_threshold;
				c.max_children = selfplay.search_config.max_children;
				c.policy_temperature = selfplay.search_config.policy_temperature;
				c.information_leak_threshold = selfplay.search_config.information_leak_threshold;
				c.tss_max_positions = selfplay.search_config.tss_max_positions;
				c.tss_table_entries = selfplay.search_config.tss_table_entries;
				const std::string &noise = selfplay.search_config.noise_type;
				if (noise != "none" && noise != "custom" && noise != "dirichlet" && noise != "gumbel")
					throw std::logic_error("GeneratorPool: unknown noise_type '" + noise + "'");
				c.noise_type = (noise == "custom") ? 1 : ((noise == "dirichlet") ? 2 : ((noise == "gumbel") ? 3 : 0));
				c.noise_weight = selfplay.search_config.noise_weight;
				c.final_selector = final_selector_id(selfplay.final_selector);
				c.use_symmetries = selfplay.use_symmetries ? 1 : 0;
				c.action_values = (selfplay.network_outputs == "pvq") ? 1 : 0;
				c.record_format = selfplay.record_format;
				// pacing only, per-game results do not depend on either (agx.h): the leaves of a batch solved in parallel, a launch's stragglers
				// put off to the next launch
				c.speculative_solver = 1;
				c.solver_yield_fraction = (c.n_games >= 64) ? 0.5f : 0.0f;
				if (game.rows != game.cols)
					throw std::logic_error("GeneratorPool: only square boards are supported");
				check(agx_engine_create(&c, &m_engine));
				check(agx_engine_buffers(m_engine, &m_buffers));
				m_games = c.n_games;
				m_match = evaluationMatches;
			}
			GeneratorPool(const GeneratorPool&) = delete;
			GeneratorPool& operator=(const GeneratorPool&) = delete;
			~GeneratorPool()
			{
				agx_engine_destroy(m_engine);
			}
			/* openings: n x AGX_OPENING_CAP uint16 ([0] = stone count, then Move::toShort words), cf. prepareOpening (utils/misc.cpp:142-170) */
			void begin(const std::vector<uint16_t> &openings, void *stream = nullptr)
			{
				if (openings.empty() || openings.size() % AGX_OPENING_CAP != 0)
					throw std::logic_error("GeneratorPool::begin: openings must hold a positive multiple of AGX_OPENING_CAP words");
				check(agx_engine_begin(m_engine, openings.data(), static_cast<int>(openings.size() / AGX_OPENING_CAP), stream));
				m_phase_started = m_skip_first_search_of_slice0 = false; // new games: every slice's cycle starts at its select stage again (generate())
			}
			/* OpeningGenerator::generate (OpeningGenerator.cpp:21-78): solver-unproven, network-balanced openings; before begin() */
			std::vector<uint16_t> generateOpenings(AGNetwork &network, int count, uint32_t seed = 0)
			{
				std::vector<uint16_t> out(static_cast<size_t>(count) * AGX_OPENING_CAP);
				check(agx_engine_generate_openings(m_engine, network.handle(), count, seed, out.data(), nullptr));
				return out;
			}
			/* Steps the pool as `slices` groups of games from now on, each on a stream that owns 1 / slices of the device's compute units
			 * (agx_stream_create_with_cu_mask), with the network's persistent grid narrowed to a slice: the slices run out of phase, the
			 * power-limited network launches never cover the whole chip at once (+10 % simulations/s on MI355X with 4 slices).  Returns the
			 * slice count in use (1 if the pool cannot be divided or the device offers no CU masks).  Self-play pools only. */
			int useChipSlices(AGNetwork &network, int slices, int instance = -1)
			{ // instance: which set of masked streams (they are cached per device, mask and instance): pools that run at the same time on one device
			  // must not share a queue — by default every call takes a set of its own
				static std::atomic<int> next_instance { 0 };
				if (instance < 0)
					instance = next_instance.fetch_add(1);
				m_slice_streams.clear();
				int cus = 0;
				if (m_match || slices <= 1 || slices > 16 || m_games % slices != 0 || agx_device_cu_count(&cus) != AGX_OK || cus < slices)
					return 1;
				const int per = cus / slices;
				for (int g = 0; g < slices; g++)
				{
					std::vector<uint32_t> mask((cus + 31) / 32, 0u);
					for (int c = g * per; c < (g + 1) * per; c++)
						mask[c / 32] |= 1u << (c % 32);
					void *s = nullptr;
					if (agx_stream_create_with_cu_mask_instance(&s, mask.data(), static_cast<int>(mask.size()), instance) != AGX_OK)
					{
						m_slice_streams.clear();
						return 1;
					}
					m_slice_streams.push_back(s);
				}
				check(agx_net_set_launch_width(network.handle(), per));
				return slices;
			}
		private:
			void run_stage(AGNetwork &network, int g, int which)
			{
				const int n = static_cast<int>(m_slice_streams.size());
				if (which == 0)
					check(agx_engine_select_solve_group(m_engine, g, n, m_slice_streams[g]));
				else if (which == 1)
					check(agx_engine_evaluate_group(m_engine, network.handle(), g, n, m_slice_streams[g]));
				else
					check(agx_engine_expand_backup_group(m_engine, g, n, m_slice_streams[g]));
			}
			static int slice_phase(int g) noexcept
			{ // stages of its NEXT cycle a slice has queued between two generate() calls
				static const int PHASES[4] = { 0, 1, 2, 1 };
				return PHASES[g % 4];
			}
			struct EventGuard
			{ // (an event must not outlive a stage that throws)
					void *event = nullptr;
					~EventGuard()
					{
						if (event != nullptr)
							agx_event_destroy(event);
					}
			};
		public:
			/* GameGenerator::generate for every game of the pool: one select -> solve -> evaluate -> expand/backup -> move step.
			 *
			 * A SLICED pool (setSlices) is left ROTATED between calls: slice g has the first slice_phase(g) = 0 / 1 / 2 / 1 stages of its next cycle
			 * queued already (slices 1 and 3 their search launch, slice 2 search + network), so a call that drains records, reads statistics or
			 * game_info, saves the games, or passes ANOTHER network sees a step boundary for slice 0 only — the network given to this call is not
			 * the one that evaluates slice 2's already-queued batch.  Callers that need step-aligned state (a network swap between training
			 * iterations, save_games, comparisons against a lock-step pool) call align() first; the next generate() re-enters the rotation. */
			void generate(AGNetwork &network, void *stream = nullptr)
			{
				if (m_slice_streams.empty())
				{
					check(agx_engine_step(m_engine, network.handle(), stream));
					if (m_pacers.empty())
						m_pacers.emplace_back(m_steps_ahead);
					m_pacers[0].step(stream);
				}
				else
				{ // The slices run a stage apart: slice g's cycle starts `phase` stages early (once, at the first call), after that every call runs one
				  // whole cycle per slice, rotated.  Slices that start together stay together while the host feeds them in step — four towers at
				  // once, the power-limited case the slicing exists to avoid (bench.py --stagger: 780 k -> 827 k simulations/s in a short window).
					const int n = static_cast<int>(m_slice_streams.size());
					if (!m_phase_started)
					{
						m_phase_started = true;
						// ... and on the DEVICE the odd slices begin when slice 0's first search launch is over (streams run their queues
						// independently: without this every slice starts its first search at the same moment, whatever the host's order)
						EventGuard first_search_done;
						for (int g = 0; g < n; g++)
						{
							if (g % 2 == 1 && first_search_done.event != nullptr)
								check(agx_stream_wait_event(m_slice_streams[g], first_search_done.event));
							for (int k = 0; k < slice_phase(g); k++)
								run_stage(network, g, k);
							if (g == 0 && n > 1)
							{
								check(agx_engine_select_solve_group(m_engine, 0, n, m_slice_streams[0])); // (slice 0's first cycle starts here; the loop below skips that stage once)
								check(agx_event_create(&first_search_done.event));
								check(agx_event_record(first_search_done.event, m_slice_streams[0]));
								m_skip_first_search_of_slice0 = true;
							}
						}
					}
					for (int g = 0; g < n; g++)
					{
						for (int k = 0; k < 3; k++)
						{
							const int which = (slice_phase(g) + k) % 3;
							if (g == 0 && which == 0 && m_skip_first_search_of_slice0)
							{
								m_skip_first_search_of_slice0 = false;
								continue;
							}
							run_stage(network, g, which);
						}
						while (static_cast<int>(m_pacers.size()) <= g)
							m_pacers.emplace_back(m_steps_ahead);
						m_pacers[g].step(m_slice_streams[g]); // the host stays two steps ahead of every slice and sleeps otherwise (HostPacer)
					}
				}
			}
			/* Brings every slice of a sliced pool to a step boundary: the stages of the cycles that generate() left begun are completed with
			 * `network` (no new cycle is started), so that records, statistics, save_games and a network swap see whole steps of every slice.  The
			 * next generate() starts the rotation again.  Nothing to do for an unsliced pool or before the first generate(). */
			void align(AGNetwork &network)
			{
				if (m_slice_streams.empty() || !m_phase_started)
					return;
				const int n = static_cast<int>(m_slice_streams.size());
				for (int g = 0; g < n; g++)
				{
					int begun = slice_phase(g);
					if (g == 0 && m_skip_first_search_of_slice0)
						begun = 1; // (only between the two halves of a first generate() that threw)
					for (int k = begun; begun > 0 && k < 3; k++)
						run_stage(network, g, k);
				}
				m_phase_started = false;
				m_skip_first_search_of_slice0 = false;
			}
			/* steps the host may run ahead of the device (0: unbounded — the launch loop then spins on a full queue); before the first generate() */
			void setHostStepsAhead(int steps) { m_steps_ahead = steps; }
			/* EvaluationGame::generate for every pair: the first players' trees with their network, then the second players' */
			void generate(AGNetwork &first, AGNetwork &second, void *stream = nullptr)
			{
				check(agx_engine_step_match(m_engine, first.handle(), second.handle(), stream));
			}
			/* per pair: games won / drawn / lost by the first player, games finished */
			std::vector<int> getMatchResults() const
			{
				std::vector<int> out(static_cast<size_t>(m_buffers.slots) * 4);
				check(agx_engine_match_results(m_engine, out.data(), static_cast<int>(out.size() / 4)));
				return out;
			}
			/* the same totals over all pairs — { won, drawn, lost by the first player, games finished } — summed on the device behind the
			 * work `stream` holds: 32 bytes for a polling loop (agx_engine_match_summary) */
			std::array<long long, 4> matchSummary(void *stream = nullptr) const
			{
				std::array<long long, 4> out { };
				check(agx_engine_match_summary(m_engine, out.data(), stream));
				return out;
			}
			/* pair results logged on the device (agx_engine_match_track_pairs): before the pool's openings are set; `capacity` log entries */
			void trackPairs(int capacity)
			{
				check(agx_engine_match_track_pairs(m_engine, capacity));
				m_pair_capacity = capacity;
			}
			/* the log's entries from `first` on, in log order (launch, then pair), and the totals (agx_engine_match_pair_results: histogram of
			 * the points, results seen, flags, log launches); max_entries = 0: the totals alone */
			std::vector<AgxPairResult> pairResults(int first, int max_entries, std::array<long long, 8> &totals, void *stream = nullptr) const
			{
				std::vector<AgxPairResult> out(static_cast<size_t>(max_entries > 0 ? max_entries : 0));
				check(agx_engine_match_pair_results(m_engine, first, out.empty() ? nullptr : out.data(), static_cast<int>(out.size()), totals.data(), stream));
				const long long logged = std::min<long long>(totals[5], m_pair_capacity); // (a full log counts on: flag 1 in totals[6])
				const long long end = std::min<long long>(logged, static_cast<long long>(first) + static_cast<long long>(out.size()));
				out.resize(static_cast<size_t>(end > first ? end - first : 0));
				return out;
			}
			/* what player 0 (first) / 1 (second) of an evaluation pool searches with (evaluation/Player.cpp:64-81: every Player takes these from
			 * its own SelfplayConfig); both start with the pool's configuration.  setPlayerSearch holds from the next generate() on. */
			AgxPlayerSearch playerSearch(int player) const
			{
				AgxPlayerSearch out { };
				check(agx_engine_player_search(m_engine, player, &out));
				return out;
			}
			void setPlayerSearch(int player, const AgxPlayerSearch &search)
			{
				check(agx_engine_set_player_search(m_engine, player, &search));
			}
			/* the three stages separately (Search::select+solve+scheduleToNN / NNEvaluator::evaluateGraph / generateEdges+expand+backup) */
			void selectSolveSchedule(void *stream = nullptr)
			{
				check(agx_engine_select_solve(m_engine, stream));
			}
			void evaluateGraph(AGNetwork &network, void *stream = nullptr)
			{
				check(agx_engine_evaluate(m_engine, network.handle(), stream));
			}
			void expandBackup(void *stream = nullptr)
			{
				check(agx_engine_expand_backup(m_engine, stream));
			}
			AgxEngineStats getStats() const
			{
				AgxEngineStats s;
				check(agx_engine_stats(m_engine, &s));
				return s;
			}
			/* Tree::getInfo({}) of one game */
			AgxGameInfo getInfo(int game, std::vector<AgxEdgeView> *root_edges = nullptr, std::vector<uint8_t> *board = nullptr) const
			{
				AgxGameInfo info;
				std::vector<AgxEdgeView> edges(400);
				std::vector<uint8_t> b(m_buffers.cells);
				check(agx_engine_game_info(m_engine, game, &info, b.data(), edges.data(), static_cast<int>(edges.size())));
				if (root_edges != nullptr)
					root_edges->assign(edges.begin(), edges.begin() + info.root_edges);
				if (board != nullptr)
					*board = b;
				return info;
			}
			/* Tree::setBoard(board, signToMove, forceRemoveRootNode) for one game driven from outside (board: one byte per cell, 0 / 1 / 2) */
			void setBoard(int game, const std::vector<uint8_t> &board, int signToMove, bool forceRemoveRootNode = false, void *stream = nullptr)
			{
				check(agx_engine_set_board_ex(m_engine, game, board.data(), signToMove, forceRemoveRootNode ? 1 : 0, stream));
			}
			/* Tree::getInfo(moves) of one game for a move path from its base board (Move::toShort words); edges (optional) receives the node's edges */
			AgxNodeView getInfo(int game, const std::vector<uint16_t> &moves, std::vector<AgxEdgeView> *edges, void *stream = nullptr) const
			{
				const int offsets[2] = { 0, static_cast<int>(moves.size()) };
				AgxNodeView view;
				std::vector<AgxEdgeView> e(edges != nullptr ? m_buffers.cells : 0);
				check(agx_engine_node_info(m_engine, game, moves.data(), offsets, 1, &view, edges != nullptr ? e.data() : nullptr, static_cast<int>(e.size()), stream));
				if (edges != nullptr)
					edges->assign(e.begin(), e.begin() + (view.found ? view.n_edges : 0));
				return view;
			}
			/* the principal variation from the node the path leads to (BestEdgeSelector at every ply, SearchEngine::getSummary): its moves */
			std::vector<uint16_t> getPrincipalVariation(int game, const std::vector<uint16_t> &moves = { }, std::vector<AgxEdgeView> *edges = nullptr,
					std::vector<AgxNodeView> *nodes = nullptr, void *stream = nullptr) const
			{
				const int cap = m_buffers.cells;
				std::vector<uint16_t> pv(cap);
				std::vector<AgxEdgeView> e(cap);
				std::vector<AgxNodeView> n(cap + 1);
				int length = 0;
				check(agx_engine_principal_variation(m_engine, game, moves.data(), static_cast<int>(moves.size()), cap, pv.data(), e.data(), n.data(), &length, stream));
				pv.resize(length);
				if (edges != nullptr)
					edges->assign(e.begin(), e.begin() + length);
				if (nodes != nullptr)
					nodes->assign(n.begin(), n.begin() + length + 1);
				return pv;
			}
			/* samples produced so far (one per played move): what GameGenerator::make_move hands to GameDataStorage */
			void getRecords(std::vector<AgxMoveRecord> &records, std::vector<AgxEdgeView> &edges) const
			{
				int nr = 0, ne = 0;
				check(agx_engine_records(m_engine, nullptr, 0, nullptr, 0, &nr, &ne));
				records.resize(nr > 0 ? nr : 1);
				edges.resize(ne > 0 ? ne : 1);
				check(agx_engine_records(m_engine, records.data(), nr, edges.data(), ne, &nr, &ne));
				records.resize(nr);
				edges.resize(ne);
			}
			/* hand-over to the game buffer: returns the samples and empties the device-side pools */
			void drainRecords(std::vector<AgxMoveRecord> &records, std::vector<AgxEdgeView> &edges)
			{
				int nr = 0, ne = 0;
				check(agx_engine_records(m_engine, nullptr, 0, nullptr, 0, &nr, &ne));
				records.resize(nr > 0 ? nr : 1);
				edges.resize(ne > 0 ? ne : 1);
				check(agx_engine_drain_records(m_engine, records.data(), static_cast<int>(records.size()), edges.data(), static_cast<int>(edges.size()), &nr, &ne));
				records.resize(nr);
				edges.resize(ne);
			}
			void addOpenings(const std::vector<uint16_t> &openings)
			{
				if (openings.empty() || openings.size() % AGX_OPENING_CAP != 0)
					throw std::logic_error("GeneratorPool::addOpenings: openings must hold a positive multiple of AGX_OPENING_CAP words");
				check(agx_engine_add_openings(m_engine, openings.data(), static_cast<int>(openings.size() / AGX_OPENING_CAP)));
			}
			const AgxEngineBuffers& buffers() const noexcept
			{
				return m_buffers;
			}
			AgxEngine* handle() const noexcept
			{
				return m_engine;
			}
	};

	/* How well a network fits a set of samples (agx.h: agx_net_score_*): the sums of AgxNetScore and the means a learning curve plots.
	 * The loss formulas are this project's own; accuracy(k) is the reference's getAccuracy (NetworkDataPack.cpp:321-345) / averageStats. */
	struct NetScore: AgxNetScore
	{
			NetScore() :
					AgxNetScore { }
			{
			}
			double policy_loss() const noexcept
			{
				return (samples > 0) ? policy_ce / static_cast<double>(samples) : 0.0;
			}
			double value_loss() const noexcept
			{
				return (samples > 0) ? value_ce / static_cast<double>(samples) : 0.0;
			}
			double q_loss() const noexcept
			{ // per cell that had an edge
				return (q_cells > 0) ? q_ce / static_cast<double>(q_cells) : 0.0;
			}
			/* fraction of the samples whose best target move is among the network's k best, k = 1 .. 4 */
			double accuracy(int k) const
			{
				if (k < 1 || k > 4)
					throw std::invalid_argument("NetScore::accuracy: k must be 1 .. 4");
				return (samples > 0) ? static_cast<double>(topk_hit[k - 1]) / static_cast<double>(samples) : 0.0;
			}
	};

	/* The training loss of the three heads and dL/dlogits in one call (agx.h: agx_head_loss_grad; device pointers, enqueued on `stream`, nothing
	 * synchronised).  The records of the n samples are added to *d_total in sample order; read it back into a NetScore for the means. */
	inline void head_loss_grad(int rows, int cols, int n, const float *d_policy_logits, const float *d_value_logits, const float *d_q_logits,
			const float *d_policy_target, const float *d_value_target, const float *d_q_target, float policy_scale, float value_scale, float q_scale,
			float *d_policy_grad, float *d_value_grad, float *d_q_grad, AgxSampleScore *d_sample_scores, AgxNetScore *d_total, void *stream = nullptr)
	{
		check(agx_head_loss_grad(rows, cols, n, d_policy_logits, d_value_logits, d_q_logits, d_policy_target, d_value_target, d_q_target, policy_scale,
				value_scale, q_scale, d_policy_grad, d_value_grad, d_q_grad, d_sample_scores, d_total, stream));
	}

	/* ... with a weight per cell for the action-value head (agx.h: agx_head_loss_grad_weighted): d_q_weight is the action_values_weight of
	 * TrainingDataset::loadBatch(samples, tensors, ...); null gives the unweighted form */
	inline void head_loss_grad(int rows, int cols, int n, const float *d_policy_logits, const float *d_value_logits, const float *d_q_logits,
			const float *d_policy_target, const float *d_value_target, const float *d_q_target, const float *d_q_weight, float policy_scale, float value_scale,
			float q_scale, float *d_policy_grad, float *d_value_grad, float *d_q_grad, AgxSampleScore *d_sample_scores, AgxNetScore *d_total, void *stream = nullptr)
	{
		check(agx_head_loss_grad_weighted(rows, cols, n, d_policy_logits, d_value_logits, d_q_logits, d_policy_target, d_value_target, d_q_target, d_q_weight,
				policy_scale, value_scale, q_scale, d_policy_grad, d_value_grad, d_q_grad, d_sample_scores, d_total, stream));
	}

	/* The consumer of the record sink: format-201 games -> training tensors on the device (agx.h: agx_dataset_*; what the reference's
	 * dataset/torch_api.h reader does on one host thread).  Fragments are numbered like Dataset::load(i, path). */
	class TrainingDataset
	{
			AgxDataset *m_dataset = nullptr;
		public:
			TrainingDataset(int rules, int rows, int cols)
			{
				check(agx_dataset_create(rules, rows, cols, &m_dataset));
			}
			TrainingDataset(const TrainingDataset&) = delete;
			TrainingDataset& operator=(const TrainingDataset&) = delete;
			~TrainingDataset()
			{
				agx_dataset_destroy(m_dataset);
			}
			void load(int fragment, const std::string &path)
			{
				check(agx_dataset_add_fragment_file(m_dataset, fragment, path.c_str()));
			}
			void load(int fragment, const AgxGameBuffer *buffer)
			{
				check(agx_dataset_add_fragment_buffer(m_dataset, fragment, buffer));
			}
			void unload(int fragment)
			{
				check(agx_dataset_unload_fragment(m_dataset, fragment));
			}
			int numberOfGames() const
			{
				int games = 0;
				check(agx_dataset_games(m_dataset, &games));
				return games;
			}
			/* (fragment, game, samples, symmetries) per game */
			std::vector<int> sizes() const
			{
				std::vector<int> result(4 * static_cast<size_t>(numberOfGames()));
				if (!result.empty())
					check(agx_dataset_sizes(m_dataset, result.data(), static_cast<int>(result.size() / 4)));
				return result;
			}
			AgxGameBufferStats getStats() const
			{
				AgxGameBufferStats stats;
				check(agx_dataset_stats(m_dataset, &stats));
				return stats;
			}
			/* device pointers, enqueued on `stream`; d_input / d_features may be null */
			void loadBatch(const std::vector<AgxDatasetSample> &samples, void *d_input, uint32_t *d_features, float *d_policy, float *d_value, float *d_moves_left,
					float *d_action_values, int flags = 0, void *stream = nullptr)
			{
				check(agx_dataset_load_batch(m_dataset, static_cast<int>(samples.size()), samples.data(), d_input, d_features, d_policy, d_value, d_moves_left,
						d_action_values, flags, stream));
			}
			/* the extended form: every output in one struct, action_values_weight among them (may be null); flags may name the policy
			 * target (AGX_BATCH_POLICY_VISITS or AGX_BATCH_POLICY_VALUES) */
			void loadBatch(const std::vector<AgxDatasetSample> &samples, const AgxBatchTensors &tensors, int flags = 0, void *stream = nullptr)
			{
				check(agx_dataset_load_batch_ex(m_dataset, static_cast<int>(samples.size()), samples.data(), &tensors, flags, stream));
			}
			/* losses and top-k accuracy of `net` on these samples: batch, network and reductions on the device, `chunk` samples at a time
			 * (0 = 1024); waits for the result */
			NetScore score(const AGNetwork &net, const std::vector<AgxDatasetSample> &samples, int chunk = 0, void *stream = nullptr)
			{
				NetScore result;
				check(agx_net_score_dataset(net.handle(), m_dataset, static_cast<int>(samples.size()), samples.data(), chunk, &result, stream));
				return result;
			}
			/* ... against the targets of a policy flag, the action-value term weighted per cell by visits / sum of visits when q_weighted */
			NetScore score(const AGNetwork &net, const std::vector<AgxDatasetSample> &samples, int chunk, int batch_flags, bool q_weighted, void *stream = nullptr)
			{
				NetScore result;
				check(agx_net_score_dataset_ex(net.handle(), m_dataset, static_cast<int>(samples.size()), samples.data(), chunk, batch_flags, q_weighted ? 1 : 0, &result,
						stream));
				return result;
			}
			/* the positions of the samples as PositionSearcher takes them: d_boards uint8[n][rows * cols], d_signs uint8[n]; one launch on `stream` */
			void positions(const std::vector<AgxDatasetSample> &samples, uint8_t *d_boards, uint8_t *d_signs, void *stream = nullptr)
			{
				check(agx_dataset_positions(m_dataset, static_cast<int>(samples.size()), samples.data(), d_boards, d_signs, stream));
			}
			/* the samples of `fragment` searched again with `net` (searcher: PositionSearcher::handle()): the same games with fresh samples are
			 * appended to `out`; waits for `stream` */
			AgxReanalyseStats reanalyse(int fragment, AgxPositionSearcher *searcher, const AGNetwork &net, AgxGameBuffer *out, const AgxReanalyseOptions &options = { 0, 0, 0 },
					void *stream = nullptr)
			{
				AgxReanalyseStats stats;
				check(agx_dataset_reanalyse(m_dataset, fragment, searcher, net.handle(), out, &options, &stats, stream));
				return stats;
			}
			AgxDataset* handle() const noexcept
			{
				return m_dataset;
			}
	};

	class PositionSolver;

	/* Boards to policy, value and best moves on the device (agx.h: agx_position_evaluator_*): the encode launch in front of the tower, the
	 * combine launch behind it.  What AGNetwork::packInputData(index, board, signToMove) + forward + unpackOutput do for one caller at a
	 * time on the reference's host, for `capacity` positions per call; the average over several symmetries and the top-k are this
	 * project's own.  All pointers are device addresses; every call only enqueues on `stream`. */
	class PositionEvaluator
	{
			AgxPositionEvaluator *m_evaluator = nullptr;
		public:
			PositionEvaluator(int rules, int board_size, int capacity)
			{
				check(agx_position_evaluator_create(rules, board_size, capacity, &m_evaluator));
			}
			PositionEvaluator(const PositionEvaluator&) = delete;
			PositionEvaluator& operator=(const PositionEvaluator&) = delete;
			~PositionEvaluator()
			{
				agx_position_evaluator_destroy(m_evaluator);
			}
			/* feature words of every (position, symmetry) row: d_features uint32[n * popcount(symmetry_mask)][cells]; d_status may be null */
			void encode(int n, const uint8_t *d_boards, const uint8_t *d_signs, int symmetry_mask, uint32_t *d_features, int32_t *d_status = nullptr, void *stream = nullptr)
			{
				check(agx_position_evaluator_encode(m_evaluator, n, d_boards, d_signs, symmetry_mask, d_features, d_status, stream));
			}
			/* encode, tower, combine; any pointer of `out` may be null */
			void evaluate(const AGNetwork &net, int n, const uint8_t *d_boards, const uint8_t *d_signs, const AgxPositionOutputs &out, int symmetry_mask = 0x01, int flags = 0,
					int top_k = 0, void *stream = nullptr)
			{
				check(agx_position_evaluator_evaluate(m_evaluator, net.handle(), n, d_boards, d_signs, symmetry_mask, flags, top_k, &out, stream));
			}
			/* the same behind the threat solver (agx_position_evaluator_evaluate_solved): the solver's action list is the move set, a proven
			 * position gets its score's value; `solved` (may be null, as may its members) receives the solver's own outputs.  Declared below. */
			void evaluate_solved(const PositionSolver &solver, const AGNetwork &net, int n, const uint8_t *d_boards, const uint8_t *d_signs,
					const AgxPositionOutputs &out, const AgxSolvedPositions *solved = nullptr, int symmetry_mask = 0x01, int flags = 0, int top_k = 0, void *stream = nullptr);
			AgxPositionEvaluator* handle() const noexcept
			{
				return m_evaluator;
			}
	};

	/* The threat solver on boards (agx.h: agx_position_solver_*): every position solved as a fresh AlphaBetaSearch with an empty table and
	 * node limit max_positions would solve it, `capacity` positions per call, one wavefront per position.  All pointers are device
	 * addresses; solve only enqueues on `stream`. */
	class PositionSolver
	{
			AgxPositionSolver *m_solver = nullptr;
		public:
			PositionSolver(int rules, int board_size, int capacity, int max_positions = 100, uint64_t table_entries = 1u << 16, uint64_t zobrist_seed = 0x9E3779B97F4A7C15ull)
			{
				check(agx_position_solver_create(rules, board_size, capacity, max_positions, table_entries, zobrist_seed, &m_solver));
			}
			PositionSolver(const PositionSolver&) = delete;
			PositionSolver& operator=(const PositionSolver&) = delete;
			~PositionSolver()
			{
				agx_position_solver_destroy(m_solver);
			}
			/* any pointer of `out` may be null */
			void solve(int n, const uint8_t *d_boards, const uint8_t *d_signs, const AgxSolvedPositions &out, void *stream = nullptr)
			{
				check(agx_position_solver_solve(m_solver, n, d_boards, d_signs, &out, stream));
			}
			int waves() const
			{
				int w = 0;
				check(agx_position_solver_info(m_solver, &w, nullptr, nullptr));
				return w;
			}
			/* device bytes one wave owns: its table, action stack, threat-list tails, frames, undo snapshots, task, game record, feature words */
			uint64_t bytes_per_wave() const
			{
				uint64_t bytes = 0;
				check(agx_position_solver_info(m_solver, nullptr, &bytes, nullptr));
				return bytes;
			}
			/* everything the solver allocated on the device: waves x the bytes a wave owns + tables + workspace */
			uint64_t device_bytes() const
			{
				uint64_t bytes = 0;
				check(agx_position_solver_info(m_solver, nullptr, nullptr, &bytes));
				return bytes;
			}
			AgxPositionSolver* handle() const noexcept
			{
				return m_solver;
			}
	};

	inline void PositionEvaluator::evaluate_solved(const PositionSolver &solver, const AGNetwork &net, int n, const uint8_t *d_boards, const uint8_t *d_signs,
			const AgxPositionOutputs &out, const AgxSolvedPositions *solved, int symmetry_mask, int flags, int top_k, void *stream)
	{
		check(agx_position_evaluator_evaluate_solved(m_evaluator, solver.handle(), net.handle(), n, d_boards, d_signs, symmetry_mask, flags, top_k, &out, solved, stream));
	}

	/* The whole search on boards (agx.h: agx_position_searcher_*): every position searched as a fresh self-play GameGenerator would search
	 * for its first move, cfg.n_games slots that take positions off a device-side list.  All pointers are device addresses; search() returns
	 * with the stream drained, the staged calls only enqueue on `stream`. */
	class PositionSearcher
	{
			AgxPositionSearcher *m_searcher = nullptr;
		public:
			explicit PositionSearcher(const AgxEngineConfig &cfg)
			{
				check(agx_position_searcher_create(&cfg, &m_searcher));
			}
			PositionSearcher(const PositionSearcher&) = delete;
			PositionSearcher& operator=(const PositionSearcher&) = delete;
			~PositionSearcher()
			{
				agx_position_searcher_destroy(m_searcher);
			}
			/* any pointer of `out` may be null; d_serials may be null (all 0); max_steps <= 0: the default of agx.h */
			void search(const AGNetwork &net, int n, const uint8_t *d_boards, const uint8_t *d_signs, const AgxPositionSearchOutputs &out, const int32_t *d_serials = nullptr,
					int max_pv = 8, int max_steps = 0, void *stream = nullptr)
			{
				check(agx_position_searcher_search(m_searcher, net.handle(), n, d_boards, d_signs, d_serials, &out, max_pv, max_steps, stream));
			}
			void begin(int n, const uint8_t *d_boards, const uint8_t *d_signs, const AgxPositionSearchOutputs &out, const int32_t *d_serials = nullptr, int max_pv = 8,
					int max_steps = 0, void *stream = nullptr)
			{
				check(agx_position_searcher_begin(m_searcher, n, d_boards, d_signs, d_serials, &out, max_pv, max_steps, stream));
			}
			/* ... with the root of every position as a format-201 sample: sink.d_bytes[i * sink.stride ...], sink.d_sizes[i] bytes of it */
			void search(const AGNetwork &net, int n, const uint8_t *d_boards, const uint8_t *d_signs, const AgxPositionSearchOutputs &out, const AgxPositionSampleSink &sink,
					const int32_t *d_serials = nullptr, int max_pv = 8, int max_steps = 0, void *stream = nullptr)
			{
				check(agx_position_searcher_search_ex(m_searcher, net.handle(), n, d_boards, d_signs, d_serials, &out, &sink, max_pv, max_steps, stream));
			}
			void begin(int n, const uint8_t *d_boards, const uint8_t *d_signs, const AgxPositionSearchOutputs &out, const AgxPositionSampleSink &sink,
					const int32_t *d_serials = nullptr, int max_pv = 8, int max_steps = 0, void *stream = nullptr)
			{
				check(agx_position_searcher_begin_ex(m_searcher, n, d_boards, d_signs, d_serials, &out, &sink, max_pv, max_steps, stream));
			}
			void select_solve(void *stream = nullptr)
			{
				check(agx_position_searcher_select_solve(m_searcher, stream));
			}
			AgxEngineBuffers buffers() const
			{
				AgxEngineBuffers b;
				check(agx_position_searcher_buffers(m_searcher, &b));
				return b;
			}
			void evaluate(const AGNetwork &net, void *stream = nullptr)
			{
				check(agx_position_searcher_evaluate(m_searcher, net.handle(), stream));
			}
			void expand(void *stream = nullptr)
			{
				check(agx_position_searcher_expand(m_searcher, stream));
			}
			void harvest(void *stream = nullptr)
			{
				check(agx_position_searcher_harvest(m_searcher, stream));
			}
			/* the position every slot works on (-1: free), int[slots()]; waits for `stream` only */
			void slot_positions(int *h_position_of_slot, void *stream = nullptr)
			{
				check(agx_position_searcher_slots(m_searcher, stream, h_position_of_slot));
			}
			int finished(void *stream = nullptr)
			{
				int count = 0;
				check(agx_position_searcher_finished(m_searcher, stream, &count));
				return count;
			}
			int slots() const
			{
				int s = 0;
				check(agx_position_searcher_info(m_searcher, &s, nullptr));
				return s;
			}
			uint64_t device_bytes() const
			{
				uint64_t bytes = 0;
				check(agx_position_searcher_info(m_searcher, nullptr, &bytes));
				return bytes;
			}
			/* the owned engine: agx_engine_stats, agx_engine_set_max_simulations and agx_engine_set_batch_size only */
			AgxEngine* engine() const
			{
				AgxEngine *e = nullptr;
				check(agx_position_searcher_engine(m_searcher, &e));
				return e;
			}
			AgxPositionSearcher* handle() const noexcept
			{
				return m_searcher;
			}
	};
}

#endif /* AGX_HPP_ */
