/*
 * caro_hip.h -- C-ABI of libcaro_hip.so, the MI355X (gfx950) self-play engine.
 *
 * The reference (nh273/caro-ai) is pure Python: the path this library replaces
 * sits behind a Python plugin API, not an FFI.  Each entry point below names
 * the reference interface it stands in for (paths relative to the reference
 * tree).  INTEGRATION.md shows the ctypes binding a maintainer of the
 * reference would add (it is what caro_ai_amd/_lib.py does).
 *
 * Conventions
 *   - plain C types only; every `*_dev` pointer is DEVICE memory owned by the
 *     caller (e.g. a torch tensor's data_ptr()) on the engine's device;
 *     `stream` is a hipStream_t passed as void* (NULL = default stream).
 *     Calls enqueue work on `stream` and return without synchronising unless
 *     the comment says otherwise.
 *   - return value: 0 on success, negative CARO_E_* code on failure;
 *     caro_last_error() returns a message for the calling thread.
 *   - no internal threads; one engine per (process, GPU).
 *
 * Board states ("keys"), KW = caro_key_words() 64-bit words per board:
 *   connect four: KW = 1, the reference's own 63-bit state int
 *                 (lib/game/connect_four/connect_four.py:36-56).
 *   m,n,k       : KW = 2*W64, W64 = 1 (n<=8), 2 (n<=11), 4 (n<=15);
 *                 words [0,W64) = bit-plane of token 0, [W64,2*W64) = token 1,
 *                 bit i = square i of lib/game/tictactoe/tictactoe.py:14-24.
 *   caro        : the m,n,k key (same KW, same planes).
 *
 * Caro (CARO_GAME_CARO, blocked-five gomoku; an extension beyond the reference):
 *   Caro(n, k) uses TicTacToe(n, k)'s board, state key, codec, planes, action
 *   space, legality and draw.  Only the win test differs.  After the mover
 *   places a stone, look at each of the four lines through the move, over the
 *   whole line as check_win does.  The mover wins if one of those lines
 *   contains:
 *     - a run of more than k of the mover's stones (an overline always wins), or
 *     - a run of exactly k whose two end cells are not both opponent stones.
 *   A cell beyond the board edge is not a block.  So with k == n the rule is
 *   plain gomoku, and Caro(3, 3) is TicTacToe(3, 3).
 *   Bit-parallel form, for line bits f (mover) and o (opponent), with element t
 *   at bit t: W = f & f>>1 & ... & f>>(k-1).  The mover wins iff
 *   W & ~((o << 1) & (o >> k)) != 0.  Off-board cells are 0 in o, which is what
 *   makes the edge open.  Limits as for m,n,k: 2 <= k <= n <= 15, anything else
 *   is CARO_E_INVAL.
 */
#ifndef CARO_HIP_H
#define CARO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CARO_GAME_CONNECT4 0
#define CARO_GAME_MNK 1
#define CARO_GAME_CARO 2

#define CARO_E_INVAL (-22)   /* bad argument */
#define CARO_E_NOMEM (-12)   /* allocation failed */
#define CARO_E_HIP (-5)      /* HIP runtime error */
#define CARO_E_NODEV (-19)   /* no usable GPU */
#define CARO_E_STATE (-71)   /* call sequence violated */

#define CARO_RESIGNED (-2)   /* actions_dev of a ply at which the mover resigned (a refused ply is -1) */

typedef struct caro_engine caro_engine;

typedef struct caro_config {
  int32_t game_kind;          /* CARO_GAME_* */
  int32_t n, k;               /* m,n,k board side and run length (TicTacToe(n, k_to_win), tictactoe.py:27) */
  int32_t n_games;            /* G concurrent games on this GPU */
  int32_t n_stores;           /* 1: one tree per game shared by both players (utils.py:60-61);
                                 2: one tree per player (utils.py:58-59, play.py:47) */
  int32_t n_nets;             /* 1: self-play; 2: player p's leaves go to net p (utils.py:64,77-79) */
  int32_t max_batch;          /* largest mcts_batch_size that will be used */
  int32_t node_cap;           /* nodes per tree; 0 = searches_hint * max_batch * max plies bound */
  int32_t steps_before_tau_0; /* utils.py:70,97-99 */
  int32_t first_player_mode;  /* 0: all games start with player 0; 1: player 1; 2: game uid & 1 */
  float c_puct;               /* config.C_PUCT */
  double alpha, explore;      /* config.ALPHA, config.EXPLORE */
  uint64_t seed;              /* key of the generated noise / move uniforms (caro_noise.h) */
  uint64_t uid_base;          /* uid of this engine's game 0 (rank offset in multi-GPU runs) */
  uint64_t uid_stride;        /* uid += uid_stride each time a game slot is recycled (total games in flight) */
  int32_t device_id;
  int32_t evict;              /* 1: after every move drop the nodes that can no longer be reached (boards that do
                                 not contain the new root).  Result-neutral; node_cap then bounds the LIVE nodes. */
  int32_t stagger;            /* > 0: staggered mode with this many minibatches (mcts_searches) per move -- every game
                                 on its own minibatch clock, see caro_search_staggered; 0: lock-step */
  int32_t stagger_recycle;    /* staggered mode, 1: a finished game's slot restarts in-kernel (uid += uid_stride).
                                 2 (with games_limit > 0), the POOL form: a finished slot waits for the next
                                 caro_drain_parked_begin, which hands the free slots the next games of the wanted set that
                                 have not been started yet, in slot order (local index i = uid uid_base + i % n_games +
                                 (i / n_games) * uid_stride: the same set of games) -- the slots stay busy until the
                                 wanted games run out, whatever the lengths of the games a slot happened to get */
  int64_t games_limit;        /* > 0: the engine plays exactly the games with local index k * n_games + g < games_limit
                                 (slot g, its k-th game; uid = uid_base + g + k * uid_stride): a slot whose next game
                                 would lie beyond that stays finished instead of restarting, in either schedule, and
                                 slots g >= games_limit never start.  This is train.py:41-47's `for _ in
                                 range(PLAY_EPISODES)` as a property of the engine: no game outside the wanted set is
                                 ever started, so counters and tuples belong to the wanted games only.  0: no limit */
} caro_config;

const char* caro_last_error(void);
/* 100: the interface up to early stop; 101: nets of any depth (the caro_net_*_depth calls, caro_net_depth); 102: random
 * openings (caro_engine_set_openings, caro_host_open_uniform, caro_host_opening, caro_openings_batch, caro_drain_extra's
 * open_dev); 103: forced playouts (caro_engine_set_forced_playouts, caro_forced_stats, caro_host_forced_root,
 * caro_host_forced_prune); 104: the two forms of the one-wave tree kernels (caro_engine_set_kernel_form,
 * caro_engine_kernel_form); 105: first-play urgency reduction (caro_engine_set_fpu, caro_host_fpu_level); 106: virtual
 * loss (caro_engine_set_virtual_loss, caro_host_vl_level); 107: move temperature and visit-count policy targets
 * (caro_engine_set_temperature, caro_host_temperature).  No existing symbol changed its signature or meaning between
 * them.  Addendum to 107 (the number stays: callers find these by symbol lookup): the session pool, caro_pool_open,
 * caro_pool_set, caro_pool_select, caro_pool_hold; position analysis, caro_principal_lines, caro_host_line_heads;
 * session levels, caro_pool_level, caro_pool_select_budget; the two forms of the row-Winograd net kernel,
 * caro_net_set_kernel_form, caro_net_kernel_form, caro_net_last_launch_form; the fine grain of the table evaluator,
 * caro_net_create_hash_grain; paired openings for arena matches, caro_engine_set_opening_pairs. */
int caro_version(void);

/* ---- geometry of a game kind (host only, no GPU needed) ---- */
int caro_key_words(int game_kind, int n);                    /* KW */
int caro_action_space(int game_kind, int n);                 /* BaseGame.action_space */
int caro_obs_cells(int game_kind, int n);                    /* H*W of BaseGame.obs_shape */

/* ---- host-side single-state rule helpers (API-edge use by the BaseGame shim;
 *      compiled from the same caro_rules.h as the kernels; no GPU needed) ---- */
/* BaseGame.initial_state (connect_four.py:67-74, tictactoe.py:56-63) */
int caro_host_initial(int game_kind, int n, int k, uint64_t* key);
/* BaseGame.move (connect_four.py:241-265, tictactoe.py:210-235; caro: the rule above): key updated in place, *won set */
int caro_host_move(int game_kind, int n, int k, uint64_t* key, int move, int player, int* won);
/* BaseGame.possible_moves as a byte mask legal[A] (connect_four.py:157-165, tictactoe.py:137-150) */
int caro_host_legal(int game_kind, int n, int k, const uint64_t* key, uint8_t* legal);
/* BaseGame.states_to_training_batch for one state -> float32[2*H*W] */
int caro_host_encode(int game_kind, int n, int k, const uint64_t* key, int who_move, float* planes);
/* one Dirichlet row / one move uniform of the caro_noise.h spec */
int caro_host_noise_row(uint64_t seed, uint64_t uid, uint32_t ply, uint32_t sim, int A, double alpha, double* out);
double caro_host_move_uniform(uint64_t seed, uint64_t uid, uint32_t ply);
/* caro_resign_uniform of caro_noise.h: game `uid` plays through (never resigns) iff this is < playthrough */
double caro_host_resign_uniform(uint64_t seed, uint64_t uid);
/* caro_cap_uniform of caro_noise.h: ply `ply` of game `uid` is full iff this is < p_full (caro_engine_set_playout_cap) */
double caro_host_cap_uniform(uint64_t seed, uint64_t uid, uint32_t ply);
/* caro_open_uniform of caro_noise.h: the uniforms of game `uid`'s random opening (section "openings" below) */
double caro_host_open_uniform(uint64_t seed, uint64_t uid, uint32_t i);
/* The opening rule (section "openings") on the host, with the single-thread initial / legal / move / full of
 * caro_rules.h: the root of game `uid` whose first player is `first` (0 or 1) -> key_out u64[KW], *player_out (the side
 * to move there), *made_out (opening plies made).  max_plies as for caro_engine_set_openings (0: the initial position). */
int caro_host_opening(int game_kind, int n, int k, uint64_t seed, uint64_t uid, int first, int max_plies,
                      uint64_t* key_out, int* player_out, int* made_out);

/* The two rules of section "forced playouts" below on ONE root row, on the host, from the functions the kernels call.
 * caro_host_forced_root: N i32[A] (visit counts), P f32[A] (raw priors), noise f64[A] (the descent's Dirichlet row),
 * legal u8[A], explore (caro_config.explore), k -> forced_out u8[A] = 1 where the action is forced; returns the number
 * of forced actions (the descent takes the lowest of them; 0: the choice is the usual one).
 * caro_host_forced_prune: N i32[A], Q f64[A] (each edge's Q as the root level reads it), P f32[A], c_puct, k ->
 * N_out i32[A] = N'; returns b, the first maximum of N.  A row without visits has no policy: CARO_E_INVAL.
 * Both: 1 <= A <= 256, counts and their sum in [0, 2^30), k in [0, 64] (NaN: CARO_E_INVAL); a negative value is an
 * error code. */
int caro_host_forced_root(int A, const int32_t* N, const float* P, const double* noise, const uint8_t* legal,
                          double explore, double k, uint8_t* forced_out);
int caro_host_forced_prune(int A, const int32_t* N, const double* Q, const float* P, float c_puct, double k,
                           int32_t* N_out);

/* ONE level of a descent under section "first-play urgency" below, on the host, from the functions the kernels call.
 * The row: N i32[A], W f32[A], Q f32[A], P f32[A] (raw priors), strong i32[A] (the N word's strong flag), legal u8[A].
 * root != 0: the root level -- float64 scores, noise f64[A] the descent's Dirichlet row, explore; the base is the row's
 * root Q; q_up is ignored; `reduction` is r_root.  root == 0: a level below it -- float32 scores, noise may be NULL;
 * q_up is the raw Q of the edge taken one level up; `reduction` is r.  scores_out f64[A]: every action's score
 * (float32 scores widened; -infinity where illegal).  Returns the level's choice, the first maximum of the scores.
 * reduction == 0 scores the level as an engine never told of the feature does.  1 <= A <= 256, counts and their sum in
 * [0, 2^24), reduction in [0, 2] (NaN: CARO_E_INVAL); a negative value is an error code. */
int caro_host_fpu_level(int A, int root, const int32_t* N, const float* W, const float* Q, const float* P,
                        const int32_t* strong, const uint8_t* legal, const double* noise, float c_puct, double explore,
                        float q_up, double reduction, double* scores_out);

/* ONE level of a descent under section "virtual loss" below, on the host, from the function the kernels call, with the
 * counts of the rule given: c i32[A], c[a] = the earlier descents of the minibatch whose path holds this node's edge a,
 * each in [0, 64]; n_vl in [0, 16].  The row, root, noise, explore, scores_out, the return value and the other ranges are
 * those of caro_host_fpu_level (N + n_vl * c and its sum in [0, 2^24)).  With every c == 0 or n_vl == 0 the scores are
 * those of caro_host_fpu_level at reduction 0, bit for bit. */
int caro_host_vl_level(int A, int root, const int32_t* N, const float* W, const float* Q, const float* P,
                       const int32_t* strong, const uint8_t* legal, const double* noise, float c_puct, double explore,
                       const int32_t* c, int n_vl, double* scores_out);

/* T(N, tau) of section "temperature" below on ONE count row, on the host, from the functions the kernels call:
 * N i32[A], tau -> pi_out f64[A]; returns b, the first maximum of N.  1 <= A <= 256, counts and their sum in [0, 2^30),
 * tau = 0 or in [0.05, 8] (NaN or anything else: CARO_E_INVAL).  A row without visits has no policy at tau > 0
 * (CARO_E_INVAL: a refused ply); at tau = 0 it gives the one-hot at action 0.  A negative value is an error code. */
int caro_host_temperature(int A, const int32_t* N, double tau, double* pi_out);

/* ---- batched rule kernels (device) : lib/game rules over M independent boards ---- */
/* keys_dev u64[M,KW] in/out, moves_dev i32[M], players_dev i32[M] -> won_dev i32[M], full_dev i32[M] */
int caro_rules_move_batch(int game_kind, int n, int k, int64_t M, uint64_t* keys_dev, const int32_t* moves_dev,
                          const int32_t* players_dev, int32_t* won_dev, int32_t* full_dev, void* stream);
/* legal_dev u8[M,A] */
int caro_rules_legal_batch(int game_kind, int n, int k, int64_t M, const uint64_t* keys_dev, uint8_t* legal_dev,
                           void* stream);
/* planes_dev f32[M,2,H,W] */
int caro_rules_encode_batch(int game_kind, int n, int k, int64_t M, const uint64_t* keys_dev,
                            const int32_t* who_dev, float* planes_dev, void* stream);
/* device form of the noise spec: out_dev f64[M,A] rows keyed (seed, uid[m], ply[m], sim[m]) */
int caro_noise_batch(uint64_t seed, int64_t M, int A, double alpha, const uint64_t* uid_dev, const uint32_t* ply_dev,
                     const uint32_t* sim_dev, double* out_dev, void* stream);

/* the opening rule on the device, one game per thread -- the function the engine calls where a game starts: uid_dev
 * u64[M], first_dev i32[M] (0 or 1) -> keys_dev u64[M,KW], players_dev i32[M], made_dev i32[M]; arguments as for
 * caro_host_opening */
int caro_openings_batch(int game_kind, int n, int k, uint64_t seed, int max_plies, int64_t M, const uint64_t* uid_dev,
                        const int32_t* first_dev, uint64_t* keys_dev, int32_t* players_dev, int32_t* made_dev,
                        void* stream);

/* ---- engine: G concurrent games = G x play_game (lib/utils.py:25-108) ---- */
/* replaces MCTS.__init__ (lib/mcts.py:27-37) for every tree of every game */
int caro_engine_create(const caro_config* cfg, caro_engine** out);
void caro_engine_destroy(caro_engine* h);
/* A NEW RUN on an existing engine, in place of destroy + create (train.py:185-193 builds its store once and plays
 * every self-play call on it; here the gigabytes of tree tables are kept and only cleared): every game restarts from
 * the initial position with empty trees, zero counters, fresh minibatch clocks and no parked games -- the state
 * caro_engine_create leaves behind, so a restarted engine plays bit for bit what a fresh engine of the same
 * configuration plays.  `cfg` must agree with the engine in everything that shapes its memory (game_kind, n, k,
 * n_games, n_stores, n_nets, max_batch, node_cap, evict, device_id, staggered or not); taken afresh from it are
 * seed, uid_base, uid_stride, games_limit, steps_before_tau_0, first_player_mode, c_puct, alpha, explore, stagger
 * (the number of minibatches per move) and stagger_recycle.  Works on lock-step and staggered engines; refuses
 * (CARO_E_STATE) while a drain or a select is pending.  Enqueues on `stream`, does not synchronise. */
int caro_engine_restart(caro_engine* h, const caro_config* cfg, void* stream);
/* (re)start every game from the initial position with an empty tree: utils.py:58-73 / MCTS.clear (mcts.py:39-43).
 * first_player_dev: i32[G] or NULL (use first_player_mode). */
int caro_reset_games(caro_engine* h, const int32_t* first_player_dev, void* stream);
/* force game positions (tests, MCTS shim): root keys u64[G,KW], players i32[G]; trees are kept */
int caro_set_roots(caro_engine* h, const uint64_t* keys_dev, const int32_t* players_dev, void* stream);

/* One search_minibatch (lib/mcts.py:248-287), first half, for every live game:
 * `batch` find_leaf descents per game on the frozen tree (mcts.py:97-148: root
 * noise :48-62, PUCT :64-84, mask :86-95, first-max argmax :136, game.move :138,
 * terminal values :140-146), de-duplication of new leaves (:272-278), and the
 * NN planes of the unique leaves (game.states_to_training_batch) written as
 * dense rows into planes_dev f32[>= G*batch, 2, H, W]: rows [0,L0) feed net 0,
 * rows [L0, L0+L1) feed net 1.
 * noise_dev: f64[G, batch, A] explicit Dirichlet rows for this minibatch, or
 * NULL to generate them on device from (seed, uid, ply, sim = mb_index*batch + b).
 * leaf_keys_dev (optional, may be NULL): u64[>= G*batch, KW] keys of the rows. */
int caro_select(caro_engine* h, int batch, int mb_index, const double* noise_dev, float* planes_dev,
                uint64_t* leaf_keys_dev, void* stream);
/* MCTS.find_leaf (lib/mcts.py:97-148) of descent `b` of game `game` of the pending select:
 * info_dev i32[4] = (status 0 dropped duplicate / 1 terminal / 2 new leaf, path length, player at the leaf, -),
 * value_dev f32[1] (terminal value), leaf_key_dev u64[KW], path_keys_dev u64[maxd,KW] (the `states` list),
 * path_actions_dev i32[maxd] (the `actions` list); maxd = H*W. */
int caro_get_descent(caro_engine* h, int game, int b, int32_t* info_dev, float* value_dev, uint64_t* leaf_key_dev,
                     uint64_t* path_keys_dev, int32_t* path_actions_dev, void* stream);
/* drop a pending select without expanding (find_leaf alone does not modify the tree) */
int caro_select_cancel(caro_engine* h);
/* Blocks until the select on `stream` has finished; counts[0..1] = L0, L1. */
int caro_leaf_counts(caro_engine* h, int32_t counts[2], void* stream);
/* Device address of the two leaf counts {L0, L1} (i32[2], engine-owned), so that a consumer kernel
 * (caro_net_forward) can read them without a host round trip. */
int caro_leaf_counts_dev(caro_engine* h, const int32_t** counts_dev);
/* Second half (mcts.py:281-287): _create_node (:178-190) for every unique leaf
 * with prior row probs_dev f32[L, A] (softmax ALREADY applied, mcts.py:216) and
 * _backup (:225-246) of terminals (sim order) then new leaves (first-seen
 * order) with values_dev f32[L] (mcts.py:217). Rows are those of caro_select.
 * BUFFER SIZES: probs_dev and values_dev must be ALLOCATED for n_games * max_batch rows (the size of the planes buffer
 * handed to caro_select), whatever L is: the kernel requests a game's value rows before it knows the game's leaf
 * count (one memory latency less per minibatch), so it reads up to max_batch - 1 rows past the last leaf row --
 * never past row n_games * max_batch.  Rows >= L are read and ignored; they need not be initialised. */
int caro_expand_backup(caro_engine* h, const float* probs_dev, const float* values_dev, void* stream);

/* get_policy_value (lib/mcts.py:289-313) of every game's root with the tau the
 * game is in: pi_dev f64[G, A]; counts_dev i32[G, A] (root N) optional. */
int caro_policy(caro_engine* h, double* pi_dev, int32_t* counts_dev, void* stream);
/* One ply of play_game for every live game (utils.py:80-99): pi, history row,
 * np.random.choice via inverse CDF of a uniform (uniforms_dev f64[G], or NULL =
 * generated), game.move, win / draw detection, tau switch.
 * Optional outputs (may be NULL): actions_dev i32[G] (-1 for finished games),
 * done_dev i32[G] (1 once the game is over), result_dev i32[G] (net1_result). */
int caro_step(caro_engine* h, const double* uniforms_dev, int32_t* actions_dev, int32_t* done_dev,
              int32_t* result_dev, void* stream);
/* Replay emission (utils.py:101-106) for finished games, in game order, each
 * game's plies last-to-first exactly as the reference appends them:
 *   states_dev u64[cap,KW], players_dev i32[cap], pi_dev f64[cap,A], z_dev i32[cap]
 * and one record per drained game: games_dev i64[G,4] = (uid, first_player, net1_result, steps).
 * Drained slots restart as new games (uid += uid_stride) when `recycle` != 0,
 * otherwise they stay finished.  Synchronises; *n_tuples / *n_games set on return. */
int caro_drain_tuples(caro_engine* h, int64_t cap, uint64_t* states_dev, int32_t* players_dev, double* pi_dev,
                      int32_t* z_dev, int64_t* games_dev, int recycle, int64_t* n_tuples, int64_t* n_games,
                      void* stream);
/* The same drain in two halves for host loops that must not leave the GPU idle (the reference's loop appends to
 * its deque right away, utils.py:101-106; here the rows of move k are handed over while move k+1 is searched):
 * _begin enqueues the kernels and returns at once; _end waits for the two totals only.  The output buffers must
 * not be touched between the two calls, and their rows are valid for anything enqueued before the next _begin. */
int caro_drain_tuples_begin(caro_engine* h, int64_t cap, uint64_t* states_dev, int32_t* players_dev, double* pi_dev,
                            int32_t* z_dev, int64_t* games_dev, int recycle, void* stream);
int caro_drain_tuples_end(caro_engine* h, int64_t* n_tuples, int64_t* n_games);

/* ---- resignation (an extension beyond the reference, whose play_game has none; OFF unless this is called) ----
 * Root Q of a ply.  After the ply's search let `best` be the first maximum of the root's visit counts (the tau = 0
 * argmax of lib/mcts.py:305-311) and q that edge's Q as the root level of a descent reads it: W / N in float64 while
 * the N word's strong flag is clear, otherwise the float32 Q word widened to double (0 if the edge has no visits).
 * It is the mover's view, and the oracle's get_node(root)["Q"][best].
 * Resignation.  Game `uid` PLAYS THROUGH iff the uniform caro_resign_uniform of caro_noise.h at (seed, uid) is below
 * `playthrough`; any other game's mover resigns at a ply whose q < threshold (strict, in double):
 *   - the ply's tuple (root, player, pi as computed) is recorded as usual, and no move is made;
 *   - the game is over and the mover loses: final_r = -1, so the drain's z is -1 on the resigner's (last) tuple and
 *     alternates from there; net1_result = -1 if player 0 resigned, +1 otherwise;
 *   - caro_step / caro_search_move: done_dev = 1, actions_dev = CARO_RESIGNED;
 *   - the game's tuple count (the rows a drain hands out, caro_get_roots' ply) includes the resignation ply;
 *     caro_get_roots reports the position the mover resigned in (unchanged by the ply) and the resigner as the player
 *     to move; the record's steps field is not advanced (as for a winning ply), so a game has steps + 1 tuples;
 *   - counters[6] (plies) and counters[7] (finished games) count the ply and the game;
 *   - a refused ply (zero root visits) is never a resignation.
 * threshold = -1 never fires (Q >= -1): recording alone.
 * caro_engine_set_resign: threshold in [-1, 1], playthrough in [0, 1] (NaN or anything else: CARO_E_INVAL).  Takes
 * effect at the next ply of every game and survives caro_engine_restart.  From the first successful call on the
 * engine records the root Q of every ply it makes (a device allocation of G x max plies doubles, and its parked copy in
 * staggered mode); before it, no ply loads anything for it.  Synchronises (first call only).  Plies made before
 * the first call have no root Q: call it before the games it is meant for start.  A drain enqueued before it keeps
 * the form it was enqueued in. */
int caro_engine_set_resign(caro_engine* h, double threshold, double playthrough);
/* caro_drain_tuples_begin / caro_drain_parked_begin that also hand out each tuple's root Q, root_q_dev f64[cap], in
 * the drain's tuple order (root_q_dev NULL: the plain begin).  A non-NULL root_q_dev before caro_engine_set_resign
 * is CARO_E_STATE.  Finish with caro_drain_tuples_end. */
int caro_drain_tuples_begin_q(caro_engine* h, int64_t cap, uint64_t* states_dev, int32_t* players_dev, double* pi_dev,
                              int32_t* z_dev, int64_t* games_dev, int recycle, double* root_q_dev, void* stream);
int caro_drain_parked_begin_q(caro_engine* h, int64_t cap, uint64_t* states_dev, int32_t* players_dev, double* pi_dev,
                              int32_t* z_dev, int64_t* games_dev, double* root_q_dev, void* stream);

/* ---- playout cap randomization (KataGo, Wu 2019; an extension beyond the reference, whose play_game searches every
 * ply alike; OFF unless caro_engine_set_playout_cap is called) ----
 * Class of a ply.  Every ply is FULL or FAST.  The class is decided once, when the ply starts: at a game's first ply
 * (caro_reset_games, caro_engine_create / caro_engine_restart, a drain's recycle, a staggered slot's restart or hand-out)
 * and right after every move that does not end the game.  Ply `ply` of game `uid` is full iff the uniform
 * caro_cap_uniform of caro_noise.h at (seed, uid, ply) is < p_full, otherwise fast.
 *   - a full ply runs the engine's usual minibatch count: caro_config.stagger in staggered mode, the caller's
 *     `searches` in lock-step (caro_search_batch / caro_search_move);
 *   - a fast ply runs `fast` minibatches, min(fast, searches) in lock-step: from minibatch `fast` on it selects nothing
 *     (zero leaves, as a finished game).  It uses the same noise keys (seed, uid, ply, sim = minibatch x batch + b),
 *     the same tau rule and the same tree, which carries over to the next ply as usual;
 *   - every ply records its class, 1 = full, 0 = fast, handed out per tuple by the _x drains below.  Drains still hand
 *     out every ply: which tuples to train on is the caller's choice;
 *   - resignation, when on, applies at every ply, fast or full.
 * caro_engine_set_playout_cap: p_full in [0, 1] (NaN: CARO_E_INVAL); fast >= 2 (a fast first ply must expand its root:
 * the searches >= 2 note at caro_search_batch) and, in staggered mode, fast <= caro_config.stagger (CARO_E_INVAL);
 * CARO_E_STATE while a caro_select or a drain is pending.  A call applies to the plies that start after it and to
 * every ply that has not run a minibatch yet (a fresh engine's first plies; in lock-step every game's current ply
 * between a move and the next search); a ply that has run one keeps its class.  The setting survives
 * caro_engine_restart.  The first successful call allocates G bytes of classes and G x max plies of flags (and their
 * parked copy in staggered mode); before it no ply loads or stores anything for them.  Synchronises.
 * p_full = 1 records the flags and changes nothing else. */
int caro_engine_set_playout_cap(caro_engine* h, double p_full, int fast);
/* caro_drain_tuples_begin_q / caro_drain_parked_begin_q that also hand out each tuple's class, full_dev u8[cap]
 * (1 = full ply), in the drain's tuple order (full_dev NULL: the _q begin).  A non-NULL full_dev before
 * caro_engine_set_playout_cap is CARO_E_STATE.  Finish with caro_drain_tuples_end. */
int caro_drain_tuples_begin_x(caro_engine* h, int64_t cap, uint64_t* states_dev, int32_t* players_dev, double* pi_dev,
                              int32_t* z_dev, int64_t* games_dev, int recycle, double* root_q_dev, uint8_t* full_dev,
                              void* stream);
int caro_drain_parked_begin_x(caro_engine* h, int64_t cap, uint64_t* states_dev, int32_t* players_dev, double* pi_dev,
                              int32_t* z_dev, int64_t* games_dev, double* root_q_dev, uint8_t* full_dev, void* stream);

/* ---- early stop of decided tau = 0 plies ("smart pruning" of match engines; an extension beyond the reference, whose
 * search always spends its budget; OFF unless caro_engine_set_early_stop is called) ----
 * Budget.  M = the minibatches the ply would run without this feature: caro_config.stagger in staggered mode, the
 * caller's `searches` in caro_search_batch / caro_search_move; for a fast ply of the playout cap, `fast`
 * (min(fast, searches) in lock-step).  B = the `batch` of the search call.
 * Where it applies.  Only at a ply whose tau is 0 (steps_before_tau_0 == 0 or step >= steps_before_tau_0, the test the
 * ply itself makes).  A tau = 1 ply is never cut: its pi is the visit distribution and would change.
 * Decided.  Let m be the number of the ply's minibatches that have been backed up, and N the root's visit counts in the
 * mover's tree (the tree the ply reads: store `player` with two stores) as the descents of minibatch index m see them at
 * the root level, i.e. after those m backups, carried visits included.  best = first maximum of N, n1 = N[best],
 * n2 = the largest N[a] over a != best (0 if there is none; an absent or unexpanded root counts as all zeros).
 * The ply is DECIDED AT m iff min_minibatches <= m <= M - 2 and n1 - n2 > (M - m) * B (integers, strict).
 * Effect.  The first m at which the ply is decided ends its search one minibatch later: the minibatch of index m, whose
 * descents are the ones that saw N, is selected, evaluated and backed up as usual, and then the ply is made.  A decided ply
 * thus runs m + 1 <= M - 1 minibatches, with the noise keys (seed, uid, ply, sim = minibatch * B + b), the tau rule and the
 * tree of an uncut ply; the tree carries over as usual.  (M - m) * B counts the simulations of minibatches m .. M - 1, the
 * one in flight included, and a simulation adds at most one visit to one root edge, so the first maximum at the ply is
 * `best` whatever those simulations do: the move and the tuple (state, player, pi) of a decided ply are those the full
 * budget would have produced from the same tree.  What differs from an uncut game is everything after it (a smaller
 * carried tree) and the ply's root Q.
 *   - staggered mode: the ply is due when its clock reaches the budget or the ply is decided;
 *   - lock-step: a decided game selects nothing from minibatch index m + 1 on (zero leaves, as a finished game or a fast
 *     ply beyond `fast`); all games still wait for the slowest, so lock-step gains nothing;
 *   - resignation, when on, applies at the ply as always (q of `best` from the cut search); the playout cap sets M per
 *     ply, and a fast ply can be cut too (m <= M - 2: never with fast = 2); games_limit, restarts, the pool form and
 *     eviction are unchanged;
 *   - the step-wise entry points (caro_select with a caller-chosen mb_index) know no budget: they never decide a ply
 *     and never skip one, and record mb_index + 1 of the ply's last caro_select;
 *   - lock-step: the rule holds per search call.  A second caro_search_batch on the same roots before the ply starts
 *     undecided at its minibatch 0 with its own `searches` as M, and the ply records the count of its last call.
 * Recording.  From the first successful call on, every ply records how many minibatches it ran (u16), handed out per
 * tuple by the _ex drains below.  (A ply in flight at that first call: staggered, its clock; lock-step, the minibatches
 * selected after the call.)
 * caro_engine_set_early_stop: min_minibatches >= 1 (CARO_E_INVAL otherwise); a value > M - 2 never fires and only
 * records; CARO_E_STATE while a caro_select or a drain is pending.  Takes effect for every ply at its next root-level
 * test and survives caro_engine_restart.  The first successful call allocates G bytes + G u16 and G x max plies u16
 * (and their parked copy in staggered mode); before it no kernel loads or stores anything for the feature.
 * Synchronises. */
int caro_engine_set_early_stop(caro_engine* h, int min_minibatches);

/* ---- openings: self-play games that start from random openings (an extension beyond the reference, whose play_game
 * always starts from the empty board; OFF unless caro_engine_set_openings is called with max_plies > 0) ----
 * caro_engine_set_openings(h, max_plies) sets the largest opening length.  max_plies = 0 means off.
 * When a game starts.  The starts are a reset, a restart, a drain recycle, a staggered slot's restart, and a pool
 * hand-out.  The first player fp is chosen as today (first_player_dev[g], else first_mode).  Then, with u(i) standing
 * for caro_open_uniform of include/caro_noise.h at (seed, uid, i):
 *   1. r = min(max_plies, floor(u(0) * (max_plies + 1))).
 *   2. For i = 0 ... r-1:
 *        - Let a_0 < ... < a_{L-1} be the legal actions of the position.
 *        - Let j = min(L-1, floor(u(1 + i) * L)).
 *        - Try a_j for the side to move.
 *        - If the move wins, or leaves a board that is full, the opening ends and the move is NOT made.
 *        - Otherwise the move is made and the side flips.
 *   3. The game's root is that position.  Its player is the side to move there.
 * The uniform.  caro_open_uniform is a function of include/caro_noise.h with its own domain tag ("open"), built like
 * caro_cap_uniform.  No other stream changes.
 * What opening plies are not.
 *   - They are not searched and are not tuples.
 *   - They do not count.  ply, step, the noise keys (seed, uid, ply, sim), the tau rule, the playout-cap class, the
 *     history rows and `steps` all number the SEARCHED plies from 0, exactly as if the game had been handed that root.
 *   - `first` as drained is the mover of tuple 0.
 *   - `result` keeps its meaning: +1 if player 0 wins.
 * Recorded.  The number of opening plies actually made is recorded per game.  It is handed out per tuple as the
 * optional int16_t* open_dev field at the end of caro_drain_extra; asking for it before the first call with
 * max_plies > 0 is CARO_E_STATE.  The struct starts with its own size, so no new drain entry point is needed.
 * A set call also (re)opens every game that has not run a minibatch yet:
 *   - staggered: lm == 0 && pend == 0 && ply == 0 (the game's clock at 0, nothing pending, no ply made);
 *   - lock-step: all games, when fresh (no caro_select / search since the last reset or ply, no ply made, roots not
 *     placed by caro_set_roots since the last reset or ply).
 * So a fresh engine's first games follow the rule.  Games in flight keep their roots.
 * Lifetime and scope.
 *   - caro_engine_restart keeps the setting.
 *   - caro_set_roots is not a game start and never opens.
 *   - Session and MCTS never use it.  Arena games (utils.play_games with two nets, train.evaluate, play.py) use it only
 *     when asked to, together with caro_engine_set_opening_pairs below.
 *   - Resignation, playout cap and early stop apply unchanged from tuple 0 on.
 * Limits.  0 <= max_plies <= 64 and max_plies < A, with A read as the number of board cells (caro_obs_cells: A itself for
 * m,n,k and caro; 42 for connect four, whose A = 7 counts columns and would rule out openings longer than six plies).
 * Anything else is CARO_E_INVAL.  CARO_E_STATE while a caro_select or a drain is pending.  The first call with
 * max_plies > 0 allocates G (staggered: 2 G) int16 counts; before it no game start loads or stores anything for the
 * feature, and a call with 0 on such an engine does nothing.  Synchronises. */
int caro_engine_set_openings(caro_engine* h, int max_plies);
/* Paired openings, for matches between two nets.  With on = 1 every game start evaluates the rule above at key uid >> 1
 * in place of uid: both draws of caro_open_uniform at (seed, key, i), the length and the plies.  Nothing else changes.  The
 * first player is chosen as today; the noise keys, the move uniform and the cap / resign keys stay on uid.  So games 2j
 * and 2j + 1 make the same opening plies and then search with independent noise.  With first_player_mode 2
 * (fp = uid & 1) their roots are colour-swapped twins: the same stones with the players exchanged, and the opposite
 * mover.  Each net of an arena engine therefore meets the same position once from each side, an unbalanced opening
 * cancels inside its pair, and the pair is the unit of the match statistics (caro_ai_amd/match_stats.py).
 *   - on = 0 puts the plain key back.  CARO_E_INVAL for any other value.
 *   - CARO_E_STATE while a caro_select or a drain is pending.
 *   - CARO_E_STATE on an engine whose first_player_mode is not 2, where the twin property would silently not hold;
 *     caro_engine_restart refuses such a mode while the flag is on.
 *   - The call (re)opens the games that have not run a minibatch yet, exactly as caro_engine_set_openings does, so the
 *     two calls may come in either order.  caro_engine_restart keeps the flag.
 *   - With max_plies = 0 the flag changes nothing, and an engine whose openings were never on loads and stores nothing
 *     for it.
 *   - caro_openings_batch and caro_host_opening take the key as their uid: pass uid >> 1 for the paired form.
 * Synchronises. */
int caro_engine_set_opening_pairs(caro_engine* h, int on);

/* ---- forced playouts and policy target pruning (KataGo, Wu 2019, the second half of the section the playout cap comes
 * from; an extension beyond the reference, whose search follows PUCT alone and whose targets are the raw visit
 * distribution; OFF unless caro_engine_set_forced_playouts is called with k > 0) ----
 * With Dirichlet noise at the root, a move the noise proposed usually gets a visit or two and is then abandoned, so the net
 * never learns whether it was good.  FORCING makes every visited root child receive a minimum number of visits that grows
 * with its prior and with the root's total.  Those visits would bias the policy target, so at the ply PRUNING takes them out
 * of the tuple's pi again where PUCT would not have spent them, and drops children left with one visit.
 * Where neither applies.  A ply classed FAST by the playout cap is neither forced nor pruned: its pi is not a training
 * tuple.  A tau = 0 ply is not pruned and keeps its one-hot pi.
 * Forcing applies at the root level of every descent (caro_select, caro_search_batch / caro_search_move,
 * caro_search_staggered alike); nothing below the root changes.  With n_a = N[a], T = the sum of N over the row and prob_a
 * the float64 noised prior exactly as the root score forms it,
 *   prob_a = (double)(float)((float)(1 - explore) * P[a]) + explore * nz[a],
 * action a is FORCED iff all of these hold:
 *   - a is legal;
 *   - n_a > 0;
 *   - (double)n_a * (double)n_a < (k * prob_a) * (double)T, evaluated in float64, in that order, with no contraction.
 * A forced action's score is +infinity.  The first-maximum reduction of the root level then picks the lowest forced
 * action.  When no action is forced, the choice is the usual one.
 * Pruning applies at the ply (caro_step, caro_search_move, the staggered ply), at a tau = 1 ply that is not fast, after the
 * root's N row is read.  Definitions:
 *   - b = first maximum of N; T = the sum of N; sq = SQRT((double)T); c = (double)c_puct, where SQRT is caro_sqrt of
 *     include/caro_noise.h, the correctly rounded float64 square root;
 *   - Q_a = the edge's Q as the root level of a descent reads it (section "resignation": W / N in float64 while the N
 *     word's strong flag is clear, otherwise the float32 Q word widened; 0 without visits);
 *   - P_a = (double) of the raw float32 prior, with no noise and no keep factor;
 *   - S* = Q_b + ((c * P_b) * sq) / (double)(1 + N_b).
 * For every a != b with N_a > 0:
 *   1. F_a = (int)SQRT((k * P_a) * (double)T).
 *   2. N'_a = the smallest integer n in [max(0, N_a - F_a), N_a] with Q_a + ((c * P_a) * sq) / (double)(1 + n) < S*.
 *   3. If no such n exists, N'_a = N_a.
 *   4. If N'_a = 1, then N'_a becomes 0.
 * N'_b = N_b, and N'_a = 0 where N_a = 0.  (The predicate is monotone in n under IEEE rounding; the library bisects.)
 * The tuple's pi, as the drains hand it out, is (double)N'_a / (double)(the sum of N').  Everything else uses the unpruned
 * counts and pi exactly as without the feature: the sampled move, the root Q and the resignation test, the recorded
 * minibatch count, the refuse rule, caro_policy.  So with the same trees a game's moves do not depend on pruning.  N'_b =
 * N_b > 0, so the sum of N' is positive wherever a ply is made.
 * Early stop.  Its bound (a simulation adds at most one visit to one root edge) still holds under forcing, and early stop
 * only cuts tau = 0 plies, which are not pruned: the two combine unchanged.  Resignation reads the unpruned row; openings
 * and the playout cap (apart from the fast plies above) apply unchanged.
 * caro_engine_set_forced_playouts(h, k): k = 0 switches the feature off (every output is then what an engine that was
 * never told of it produces); k < 0, NaN or k > 64 is CARO_E_INVAL; KataGo's value is 2.  CARO_E_STATE while a
 * caro_select or a drain is pending.  Takes effect from the next launch on and survives caro_engine_restart.  Accepted on
 * an engine with two stores as caro_engine_set_playout_cap is (each side's tree by the same rule); the arena, play.py,
 * Session and MCTS never call it.  The first call with k > 0 allocates 4 x (G + 1) 64-bit tallies; before it, and while
 * k = 0, no kernel loads or stores anything for the feature.  Synchronises.
 * caro_forced_stats: out[4] = engine-wide sums since creation or the last caro_engine_restart:
 *   [0] root descents made under the rule (the root in the tree, k > 0, not a fast ply),
 *   [1] those of them that took a forced action,
 *   [2] plies whose pi lost at least one visit to pruning,
 *   [3] visits removed (the sum over those plies of the sum of N minus the sum of N').
 * All zero on an engine that never had k > 0.  Synchronises. */
int caro_engine_set_forced_playouts(caro_engine* h, double k);
int caro_forced_stats(caro_engine* h, int64_t out[4], void* stream);

/* ---- first-play urgency reduction (KataGo, Leela Zero, Lc0, ELF; an extension beyond the reference, whose PUCT
 * scores an unvisited child with Q = 0, lib/mcts.py:79-84; OFF unless caro_engine_set_fpu is called with a positive
 * reduction) ----
 * Q = 0 means "as good as a draw".  In a position the mover is losing every visited child has Q < 0, every unvisited one
 * looks better and the search fans out over the whole row; in a winning position it never looks sideways.  The rule
 * replaces the 0 by the parent's value minus a reduction that grows with the policy mass already explored.
 * It applies at EVERY level of every descent, in every launch form (caro_select, caro_search_batch / caro_search_move,
 * caro_search_staggered alike), on the frozen tree of the minibatch.  At one level, the row is the node's N | W | Q | P
 * row as that level reads it and `legal` is the level's legality mask.  No order-dependent float sum appears below: every
 * quantity is an integer reduction or a function of one edge, so the lanes of a descent group reduce in any order.
 * Visited mass.
 *   - m_a = (int)floorf(min(max(P[a], 0.0f), 1.0f) * 4194304.0f); the factor is 2^22, the product is exact;
 *   - M = the sum of m_a over the legal a with N[a] > 0, in int32 (A <= 256: at most 2^30);
 *   - s = SQRT((double)M * 2^-22), SQRT = caro_sqrt of include/caro_noise.h.
 * Base.
 *   - At the root level: the root Q of the row (section "resignation"): the first maximum of N and that edge's Q as the
 *     root level reads it, in float64; 0 if the row has no visits.
 *   - Below the root: base = -q_up, where q_up is the stored Q of the edge this descent took one level up, exactly as
 *     that level read it, rounded to float32: below a non-root level the float32 Q word; below the root level (float)qd
 *     of the root formula (the Q word if the strong flag is set, else W / N in float64, 0 if N = 0).  It is the raw
 *     edge Q, never a substituted one: an edge with N = 0 that leads to a transposed node gives base 0.
 * Substitution, only for the legal a with N[a] == 0 (everything else in the score is untouched):
 *   - root level:   qd = base - (r_root * s), every operand float64: the product, then the difference, no contraction;
 *   - other levels: q = (float)((double)base - (r * s)), the same order, ONE rounding to float32; that float enters the
 *     float32 score q + tt.
 * Visited actions, the U term, the noise, the legality mask and the first-maximum reductions stay as they are.
 * With the other options.  A forced action still scores +infinity (a forced action has n > 0, a substituted one n = 0:
 * they never meet on one action).  Pruning, early stop, the root Q of resignation, caro_policy and the refuse rule read
 * visited edges or counts only and are unchanged.  A fast ply of the playout cap uses the rule like any other ply.
 * caro_engine_set_fpu(h, reduction, root_reduction): r and r_root, each in [0, 2] (NaN or anything else:
 * CARO_E_INVAL); 0 / 0 switches the feature off, and every output is then what an engine that was never told of it
 * produces.  CARO_E_STATE while a caro_select or a drain is pending.  Takes effect from the next launch on and survives
 * caro_engine_restart.  Accepted on an engine with two stores (each side's tree by the same rule); the arena gate,
 * play.py, Session and the MCTS shim never call it.  Nothing is allocated, and while it is off no kernel loads, stores
 * or reduces anything for it.  Synchronises when the setting changes. */
int caro_engine_set_fpu(caro_engine* h, double reduction, double root_reduction);

/* ---- virtual loss (every batched MCTS has it; an extension beyond the reference, whose B descents of a minibatch all
 * walk the same frozen tree and differ by the root's Dirichlet row alone, lib/mcts.py:272-278; OFF unless
 * caro_engine_set_virtual_loss is called with n_vl > 0) ----
 * Parameter n_vl: an integer in [0, 16]. 0 means off.
 * A minibatch of one game selects descents b = 0 .. B-1. Descent b uses noise row mb * B + b. All descents read the same
 * frozen rows of one store.
 * A board fixes its depth below the root, because each move adds one stone. A node is therefore always met at the same
 * level.
 * For descent b at node X and action a, define c = c_b(X, a). It is the number of descents b' < b of this minibatch whose
 * path contains edge (X, a). An edge counts once per path. Paths that ended in a terminal count. Paths later dropped as
 * duplicates count too. The counts depend on paths only.
 * Let v = n_vl * c. The level scores this row:
 *   - Visits. N' = N + v as an int. nsum' is the integer sum of N' over the row. The U term uses nsum' and (1 + N') where
 *     it uses nsum and (1 + N) today: SQRT((double)nsum') at the root (SQRT = caro_sqrt of include/caro_noise.h);
 *     sqrt_count((float)nsum') below the root.
 *   - Q, where v == 0. The edge's Q is exactly what the level reads today. No bit may differ.
 *   - Q, where v > 0. Let q0 be the edge's Q as the level reads it with the feature off. At the root that is the float64
 *     qd. Below the root it is the float32 Q word. It is 0 if N == 0. Then Q' = (q0 * N - v) / (N + v). Evaluate it in the
 *     level's precision: float64 at the root, float32 below. Do the product first, then the difference, then the
 *     quotient. No contraction. Convert N, v and N + v from int to that precision.
 *   - Untouched. The noise, the priors, the legality mask and the first-maximum reductions do not change.
 *   - Never in memory. Virtual visits live in registers and LDS during the select only. The level's path record carries
 *     the real N and W words of the chosen edge. expand_preload and the backup rely on them. caro_lookup_nodes
 *     after a select shows the frozen rows.
 * With the other options:
 *   - First-play urgency. The visited mass and the base are formed from the real row, as today. The substitution applies
 *     to legal actions with N' == 0. An action with N == 0 and v > 0 has Q' = -1 by the formula. The q_up handed to the
 *     next level is the raw Q as read, as today.
 *   - Forced playouts. fp_forced sees N' and nsum'. The forced and pruned tallies and the pruning of pi read real
 *     counts.
 *   - Early stop, resignation's root Q, caro_policy, the refuse rule. They read the real row.
 *   - Playout cap. A fast ply uses the rule like any other.
 *   - Two stores. Each side's tree follows the same rule.
 *   - B == 1, or n_vl == 0. Every output is bit for bit what an engine never told of the feature produces.
 * caro_engine_set_virtual_loss(h, n_vl): CARO_E_INVAL outside [0, 16]; CARO_E_STATE while a caro_select or a drain is
 * pending.  Takes effect from the next launch on and survives caro_engine_restart.  Synchronises only when the setting
 * changes; allocates nothing.  The arena gate, play.py, Session and the MCTS shim never call it.
 * While n_vl > 0 every launch that selects B > 1 descents per game runs the virtual-loss instantiation of its kernel, in
 * which the B descents of a game take each level together; with n_vl == 0 the kernels are the ones an engine without the
 * feature runs. */
int caro_engine_set_virtual_loss(caro_engine* h, int n_vl);

/* ---- temperature: the move temperature and visit-count policy targets (the reference's get_policy_value takes any
 * tau, lib/mcts.py:305-311, but its play_game knows 1 and 0 only and trains on the vector it sampled from,
 * lib/utils.py:70-99; OFF unless caro_engine_set_temperature is called with anything but (1, 0, 0)) ----
 * Two choices that the engine made as one are set apart: how sharply a move is sampled, and what the tuple records.
 * The triple (tau_early, tau_late, visit_targets); the default (1, 0, 0) is the engine without the feature.
 * At a ply:
 *   - the ply is EARLY iff steps_before_tau_0 > 0 && step < steps_before_tau_0 (the test the ply always made: `step`
 *     counts the game's searched plies), otherwise LATE;
 *   - the MOVE temperature tau_m = tau_early at an early ply, tau_late at a late one;
 *   - the TUPLE temperature tau_t = 1 if visit_targets, otherwise tau_m.
 * T(N, tau) is the distribution of a count row N[0..A) whose integer sum tot is > 0.  Float64, in the order given, with
 * no contraction:
 *   - tau == 0: one-hot at the first maximum of N;
 *   - tau == 1: (double)N[a] / (double)tot;
 *   - otherwise, with nmax = max N: w_a = 0 where N[a] == 0; w_a = 1 where N[a] == nmax;
 *     w_a = EXP(LOG((double)N[a] / (double)nmax) / tau) elsewhere (LOG / EXP = caro_log / caro_exp of
 *     include/caro_noise.h); S = the sum of the w_a added SEQUENTIALLY in action order a = 0 .. A-1 from 0.0;
 *     pi_a = w_a / S.  (nmax^(1/tau) cancels: this is count ** (1 / tau) normalised, without the overflow.)
 * The move is caro_sample_index of include/caro_noise.h on T(N, tau_m) with the ply's move uniform u, as ever.  The tuple's pi -- h_pi, what
 * every drain hands out -- is T(N, tau_t).  caro_policy returns T(N, tau_m), the vector the ply would sample from.
 * With the other options:
 *   - Forced playouts.  Pruning applies at every ply that is not fast and whose tau_t > 0 (the "tau = 1 ply" of that
 *     section is this rule with the feature off); the tuple's pi is then T(N', tau_t).  b, T, sq, S* and F_a are formed
 *     from N as there.  The move still comes from the unpruned N.
 *   - Early stop.  A ply can be cut only if tau_m == 0 and tau_t == 0: anything else would change the tuple.  With
 *     visit_targets = 1, or a positive temperature at the ply, it never fires; it still records.
 *   - Refuse rule.  A root without visits is refused unless tau_m == 0 && tau_t == 0 and action 0 is legal (that exception
 *     is the tau = 0 case of the engine without the feature).
 *   - Unchanged: resignation's root Q, the playout-cap class, openings, first-play urgency, virtual loss, eviction,
 *     games_limit and the pool form.
 * caro_engine_set_temperature(h, tau_early, tau_late, visit_targets): each temperature is 0 or in [0.05, 8]; NaN, a
 * negative value, one in (0, 0.05) or above 8, and visit_targets outside {0, 1} are CARO_E_INVAL.  CARO_E_STATE while a
 * caro_select or a drain is pending.  The setting survives caro_engine_restart and takes effect at each game's next ply.
 * The feature is ON iff the triple is not (1, 0, 0); while it is off -- never set, or set back -- every output is bit
 * for bit what an engine that was never told of it produces.  Accepted on an engine with two stores as the other options
 * are; the arena gate, play.py, Session and the MCTS shim never call it.  Nothing is allocated, and while it is off no
 * kernel loads or computes anything for it.  Synchronises only when the setting changes. */
int caro_engine_set_temperature(caro_engine* h, double tau_early, double tau_late, int visit_targets);

/* ---- session pool: many human-vs-bot games in one lock-step engine (lib/play_session.py:7-49 keeps ONE game per
 * Session, and a chat front end keeps a dictionary of them; here a session is a game SLOT of one engine, and every bot
 * move that is due is searched in the same launches.  An extension beyond the reference; an engine on which none of
 * these four calls is made runs exactly as before) ----
 * HELD.  A slot of a lock-step engine is live (it searches and moves), finished (its game is over), or HELD: it keeps
 * its position, uid, ply and trees and takes part in nothing.  A held slot
 *   - selects no descent: it adds no leaf row, no entry of the slot list, no Dirichlet row, and its leaf count as the
 *     net kernel reads it is 0;
 *   - makes no ply (caro_step / caro_search_move: actions_dev = -1, done_dev = 1, as for a finished game) and is not
 *     evicted;
 *   - counts nothing (caro_counters) and is no live game (caro_live_games);
 *   - is never drained: the drains hand out finished games only.
 * caro_get_roots, caro_lookup_nodes, caro_tree_sizes, caro_policy read a held slot like any other.
 * The four calls stand for Session.__init__ (lib/play_session.py:8-21: a new game and an empty store),
 * Session.move_player (:23-26: the human's move changes the position the next search starts from; the store is kept),
 * and Session.move_bot (:28-36: search_batch on the session's own store, then the move) for a chosen SUBSET of the
 * sessions.
 * All four: lock-step engines with one tree and one net per game only -- CARO_E_STATE on a staggered engine, on one with
 * n_stores == 2 or n_nets == 2 (two nets: until LEVELS, below, are on), and while a caro_select or a drain is pending.  NULL handle or list, M < 0, a slot
 * outside [0, n_games), a slot named twice in one list (so M > n_games too): CARO_E_INVAL, and nothing is changed.  The
 * lists are device memory; the library copies them back to check them, so each call that takes a list synchronises
 * `stream` once before it enqueues its kernel (caro_pool_hold does not).  The first call allocates 8 x n_games bytes of
 * pinned host memory.  caro_engine_restart and caro_reset_games make every slot live again, as ever.
 *
 * caro_pool_open: for each listed slot m -- games_dev i32[M], uid_dev u64[M], first_player_dev i32[M] (0 or 1) -- every
 * key table of the slot's tree is cleared (the second table of an engine with eviction too), the node counts go to 0
 * (caro_tree_sizes included), the game is at the initial position with uid uid_dev[m], first_player_dev[m] to move,
 * ply 0, and the slot is HELD.  No opening is played (caro_engine_set_openings does not apply).  A slot may be opened
 * any number of times, whatever state it is in; afterwards it searches like a slot of a fresh engine with that uid. */
int caro_pool_open(caro_engine* h, int64_t M, const int32_t* games_dev, const uint64_t* uid_dev,
                   const int32_t* first_player_dev, void* stream);
/* caro_pool_set, the sparse caro_set_roots: for each listed slot m the root key keys_dev u64[M,KW], the player to move
 * players_dev i32[M] and ply_dev i32[M] = the moves made in the session so far, both sides counted -- the `ply` of the
 * noise key (seed, uid, ply, sim) of the searches that follow and of the ply's move uniform; 0 <= ply < board cells,
 * anything else CARO_E_INVAL.  The tree is KEPT (Session.mcts_store lives as long as the game).  The slot is HELD
 * afterwards, whatever it was.  With caro_config.evict the slot's tree is evicted against the new root in the same
 * call (the nodes whose boards do not contain it are dropped: result-neutral, as after a ply). */
int caro_pool_set(caro_engine* h, int64_t M, const int32_t* games_dev, const uint64_t* keys_dev,
                  const int32_t* players_dev, const int32_t* ply_dev, void* stream);
/* caro_pool_select: exactly the listed slots that are held become live; every other live slot becomes held; finished
 * slots (listed or not) stay finished.  M = 0 holds everything.  Between this call and caro_pool_hold the existing
 * caro_search_batch, caro_step and caro_search_move run unchanged: "every live game" is the listed subset.
 * caro_pool_hold: every live slot becomes held; a slot whose ply just ended its game stays finished (caro_pool_open
 * or caro_pool_set makes it usable again). */
int caro_pool_select(caro_engine* h, int64_t M, const int32_t* games_dev, void* stream);
int caro_pool_hold(caro_engine* h, void* stream);
/* LEVELS: a session's own strength -- how many minibatches its bot move searches, the temperature its move is sampled
 * at, which of the engine's nets evaluates its leaves -- with sessions of different levels searched in the same launches.
 * Found by symbol lookup like the four calls above (caro_version stays).  The feature is OFF until the first
 * caro_pool_level or caro_pool_select_budget that passes its checks: that call allocates 16 x n_games bytes of device
 * memory and switches it on for the life of the engine.  While it is off no kernel loads or computes anything for it and
 * every output is bit for bit what an engine never told of it produces.  Once it is on:
 *   - the pool calls take an engine with n_nets == 2 (and n_stores == 1; two stores stay refused); the net class of a
 *     slot's leaves -- on a two-net engine otherwise the player to move -- is the slot's net;
 *   - the ply's temperatures ("temperature" above) are tau_m = the slot's tau and tau_t = tau_m: the move is
 *     caro_sample_index of T(N, tau_m) at the move uniform of (seed, uid, ply), the refuse rule for a root without visits
 *     is unchanged, and caro_policy returns T(N, tau_m);
 *   - caro_engine_set_playout_cap, caro_engine_set_early_stop and caro_engine_set_temperature return CARO_E_STATE, as
 *     the two calls below do on an engine where one of those three is on (one rule for the minibatches of a ply, one
 *     temperature).
 * Both: CARO_E_STATE also on a staggered engine, with n_stores == 2, and while a caro_select or a drain is pending; the
 * slot list is checked as the other pool calls check theirs, and a call that returns an error changes nothing.
 *
 * caro_pool_level: persistent per slot -- slot games_dev[m] has its leaves evaluated by net net_dev[m] (i32, in [0,
 * n_nets)) and samples its plies at tau_dev[m] (f64, 0 or in [0.05, 8]), until the next caro_pool_level that names it.
 * caro_pool_open puts a slot back to (net 0, tau 0), which is also what every slot starts from.  M = 0 only switches the
 * feature on.  A value out of range is CARO_E_INVAL.
 * caro_pool_select_budget: caro_pool_select, and slot games_dev[m] selects descents only in the first budget_dev[m]
 * (i32, >= 1, else CARO_E_INVAL) minibatches of every caro_search_batch / caro_search_move (and of caro_select, by its
 * mb_index) that follows.  Past its budget a slot behaves in a launch as a fast ply of the playout cap past `fast`: zero
 * leaves, no slot rows, no Dirichlet rows, nothing counted; the launch still expands and backs up its last selected
 * minibatch.  A budget above the call's `searches` means `searches`.  The budget belongs to the SELECTION, not to the
 * slot: the next caro_pool_hold, caro_pool_select or caro_pool_select_budget clears all budgets.
 * caro_engine_restart and caro_reset_games leave levels on and touch neither a slot's (net, tau) nor a budget: hold or
 * select after them, as a pool does anyway. */
int caro_pool_level(caro_engine* h, int64_t M, const int32_t* games_dev, const int32_t* net_dev, const double* tau_dev,
                    void* stream);
int caro_pool_select_budget(caro_engine* h, int64_t M, const int32_t* games_dev, const int32_t* budget_dev, void* stream);

/* ---- position analysis: the top moves of a slot's searched root and the line the search expects after each (what a
 * person in front of a game bot asks for: "which moves did you consider", "give me a hint"; the reference has nothing of
 * the kind -- Session.move_bot, lib/play_session.py:28-36, keeps one number; an extension, and the second addendum to
 * 107: an engine on which it is never called runs exactly as before) ----
 * caro_principal_lines reads, for each listed slot m (games_dev i32[M]), the tree (slot, store) from the slot's current
 * root key and player to move, as caro_get_roots reports them.
 *   - The root is not a node of that tree: n_lines = 0, root_visits = -1.
 *   - Otherwise root_visits = the sum of N over the root's edges; the root's edges with N > 0 are RANKED by (N
 *     descending, action ascending); n_lines = min(top, the number of such edges).
 * Line j < n_lines:
 *   - step 0 is the j-th edge of the ranking;
 *   - step d > 0, at the node of the position after steps 0 .. d-1, is the edge with the largest N, ties to the lowest
 *     action (the first maximum: np.argmax's rule, the one a tau = 0 ply uses); it must have N > 0;
 *   - each step records the edge's raw words as caro_lookup_nodes splits them: move (the action), N, W, Q, P, strong;
 *   - the mover alternates from the root's player; the move is made with the rules of the engine's game kind (connect
 *     four, m,n,k, caro's blocked five).
 * After step d is recorded the line ENDS with the first of these that holds -- end_dev:
 *     1 WIN    the move won for its mover
 *     2 DRAW   the board is full
 *     0 DEPTH  d + 1 == depth
 *     3 LEAF   the position after the move is no node of the tree, or none of its edges has N > 0
 * len_dev = the steps recorded (>= 1).
 * Outputs: n_lines_dev i32[M], root_visits_dev i32[M], len_dev / end_dev i32[M, top], move_dev / N_dev / strong_dev
 * i32[M, top, depth], W_dev / Q_dev / P_dev f32[M, top, depth].  EVERY element of every output is written by the call
 * (the buffers need no initialisation): an unused line has len 0 and end -1, an unused step move -1, and zeros elsewhere.
 * The call READS only: no tree word, no counter and no slot state changes.  So a slot may be listed twice, and it may be
 * live, held or finished.  With caro_config.evict the slot's current table is read, as caro_lookup_nodes reads it.
 * Lock-step engines only: CARO_E_STATE on a staggered engine and while a caro_select or a drain is pending.  NULL handle
 * or pointer, M < 0, a slot outside [0, n_games), store outside [0, n_stores), top outside [1, 16], depth outside
 * [1, 64]: CARO_E_INVAL, and nothing is written.  M = 0 returns 0.  The list is device memory and is copied back to be
 * checked: the call synchronises `stream` once before it enqueues its kernel.
 * caro_host_line_heads: the ranking alone on ONE count row, on the host, from the functions the kernel calls -- N i32[A],
 * top in [1, 16] -> heads_out i32[top] = the ranked actions, -1 beyond the visited edges; returns n_lines.  heads_out[0]
 * is the first maximum of N.  1 <= A <= 256, counts in [0, 2^30); a negative value is an error code. */
int caro_principal_lines(caro_engine* h, int64_t M, const int32_t* games_dev, int store, int top, int depth,
                         int32_t* n_lines_dev, int32_t* root_visits_dev, int32_t* len_dev, int32_t* end_dev,
                         int32_t* move_dev, int32_t* N_dev, float* W_dev, float* Q_dev, float* P_dev,
                         int32_t* strong_dev, void* stream);
int caro_host_line_heads(int A, const int32_t* N, int top, int32_t* heads_out);

/* ---- form of the one-wave fused tree kernels (result-neutral; for tests and A/B measurements) ----
 * The tree kernels that run one wavefront per game (connect four at batch 8, 3 x 3 boards at batch 4, ...) exist in two
 * compiled forms.  The FULL form reads every option from the engine at run time.  The LEAN form has the opt-in
 * self-play features (resignation recording, playout cap, early stop, openings, forced playouts, first-play urgency,
 * virtual loss, temperature, session levels),
 * the second store of an arena engine and the diagnostic stamps compiled out.  Every launch picks the lean form iff the
 * engine uses none of those at that moment (a feature that was switched off again -- forced playouts with k = 0,
 * first-play urgency with 0 / 0, virtual loss with n_vl = 0, temperature with (1, 0, 0) -- no longer counts; openings count from the first call with max_plies > 0 on, since
 * the per-game opening counts are kept from then on).
 * Both forms compute the same bits; the lean one only spends fewer registers and instructions.
 * caro_engine_set_kernel_form: form 0 = automatic (the default), 1 = always the full form; anything else is
 * CARO_E_INVAL.  Takes effect from the next launch on; survives caro_engine_restart.
 * caro_engine_kernel_form: 0 (lean) or 1 (full), what the next launch would use. */
int caro_engine_set_kernel_form(caro_engine* h, int form);
int caro_engine_kernel_form(const caro_engine* h);

/* Optional per-tuple outputs of a drain, in the drain's tuple order; a NULL field is not written.  `size` =
 * sizeof(caro_drain_extra) of the caller's header: fields beyond it are taken as NULL, so the struct can grow.
 * root_q_dev f64[cap] needs caro_engine_set_resign, full_dev u8[cap] caro_engine_set_playout_cap, minibatches_dev
 * u16[cap] (minibatches the ply ran) caro_engine_set_early_stop, open_dev i16[cap] (opening plies made by the tuple's
 * game, constant within a game) caro_engine_set_openings with max_plies > 0: CARO_E_STATE before it. */
typedef struct caro_drain_extra {
  uint32_t size;
  double* root_q_dev;
  uint8_t* full_dev;
  uint16_t* minibatches_dev;
  int16_t* open_dev;
} caro_drain_extra;
/* caro_drain_tuples_begin / caro_drain_parked_begin with the optional outputs of `extra` (NULL: none).  The _q and _x
 * begins are these with the matching fields.  Finish with caro_drain_tuples_end. */
int caro_drain_tuples_begin_ex(caro_engine* h, int64_t cap, uint64_t* states_dev, int32_t* players_dev, double* pi_dev,
                               int32_t* z_dev, int64_t* games_dev, int recycle, const caro_drain_extra* extra,
                               void* stream);
int caro_drain_parked_begin_ex(caro_engine* h, int64_t cap, uint64_t* states_dev, int32_t* players_dev, double* pi_dev,
                               int32_t* z_dev, int64_t* games_dev, const caro_drain_extra* extra, void* stream);

/* counters[8] (host array): sims, levels, expansions, terminals, dropped
 * duplicates, overflows, plies, finished games.  Synchronises.
 * `overflows` counts every event after which the engine's games may no longer be the reference's: a minibatch whose
 * new nodes did not fit node_cap (its leaves are dropped), and a ply REFUSED because the root had no visits (one
 * search on an unexpanded root: lib/mcts.py:311 divides by zero there; the game is left where it was).  Every caller
 * in this package treats a non-zero value as an error. */
int caro_counters(caro_engine* h, int64_t counters[8], void* stream);
/* HIP-event timing of the path's kernels on the stream they are launched on (bench.py's live
 * roofline).  Kinds: 0 select, 1 scan+encode, 2 expand+backup, 3 step, 4 net forward (bracketed by the
 * caller with caro_profile_begin/_end around caro_net_forward); 5 / 6 calibrate the pairs themselves: a pair
 * around ONE launch of an empty kernel (E1) and a pair around TWO (E2), recorded behind every fourth sampled net
 * launch of caro_search_batch / caro_search_staggered -- a pair adds o = 2 E1 - E2 (+ the sub-microsecond gap between
 * two dependent launches) to the kernel it brackets, to be subtracted from the other kinds' averages; 7 free.
 * caro_profile_read synchronises on the recorded events; ms[] / launches[] are running totals. */
int caro_profile_enable(caro_engine* h, int on);
int caro_profile_begin(caro_engine* h, int kind, void* stream); /* returns a slot, or -1 when profiling is off */
void caro_profile_end(caro_engine* h, int slot, void* stream);
int caro_profile_read(caro_engine* h, double ms[8], int64_t launches[8], int reset);
/* diagnostics (tools/probe_select.py): per-game cycle stamps of k_select's phases; off unless enabled */
int caro_debug_stamps(caro_engine* h, int on);
int caro_debug_read(caro_engine* h, uint64_t* out_host, int64_t n_u64, void* stream);
/* diagnostic: the device's square root of a visit count (float32, `m.sqrt(sum(counts))` of lib/mcts.py:79 rounded as
   numpy does) compared with sqrtf on every integer 0..n_max (n_max <= 2^24); *bad_host = differing results (must be 0) */
int caro_debug_sqrt_check(uint32_t n_max, uint64_t* bad_host);
/* number of live (unfinished) games; synchronises */
int caro_live_games(caro_engine* h, int32_t* live, void* stream);
/* unique leaves that have been selected but not yet booked as expansions (between caro_select and
 * caro_expand_backup; in staggered mode the pending minibatch of every game).  At any point of a run
 * sims == expansions + terminals + dropped + pending (+ the leaves of overflowed minibatches); synchronises */
int caro_pending_leaves(caro_engine* h, int32_t* pending, void* stream);

/* ---- inspection (tests, MCTS shim: the four public dicts of lib/mcts.py:29-36) ---- */
/* len(MCTS) per tree: out_dev i32[G*n_stores] */
int caro_tree_sizes(caro_engine* h, int32_t* out_dev, void* stream);
/* nodes a tree HOLDS right now (= len(MCTS) without eviction; with caro_config.evict what survived the last
 * k_evict plus what the current move added -- the figure node_cap bounds): out_dev i32[G*n_stores] */
int caro_tree_live(caro_engine* h, int32_t* out_dev, void* stream);
/* look up M (game, store, key) triples: found_dev i32[M]; N i32[M,A]; W,Q,P f32[M,A]; strong i32[M,A]
 * (strong = W has absorbed a float32 net value; 0 = still an exact Python float) */
int caro_lookup_nodes(caro_engine* h, int64_t M, const int32_t* game_dev, const int32_t* store_dev,
                      const uint64_t* keys_dev, int32_t* found_dev, int32_t* N_dev, float* W_dev, float* Q_dev,
                      float* P_dev, int32_t* strong_dev, void* stream);
/* current root key / player / ply / uid of every game: keys u64[G,KW], players i32[G], ply i32[G], uid u64[G] */
int caro_get_roots(caro_engine* h, uint64_t* keys_dev, int32_t* players_dev, int32_t* ply_dev, uint64_t* uid_dev,
                   void* stream);
/* insert / overwrite nodes (MCTS shim attribute setters, lib/test_mcts.py:15-21): same layout as lookup */
int caro_poke_nodes(caro_engine* h, int64_t M, const int32_t* game_dev, const int32_t* store_dev,
                    const uint64_t* keys_dev, const int32_t* N_dev, const float* W_dev, const float* Q_dev,
                    const float* P_dev, const int32_t* strong_dev, void* stream);
/* MCTS._backup (lib/mcts.py:225-246) of ONE path on one tree: keys u64[len,KW], actions i32[len] */
int caro_backup_path(caro_engine* h, int game, int store, float value, int value_is_f32, int len,
                     const uint64_t* keys_dev, const int32_t* actions_dev, void* stream);
/* dump a whole tree (MCTS shim dict views): keys u64[cap,KW], N i32[cap,A], W/Q/P f32[cap,A], strong i32[cap,A];
 * *n_nodes set on return (synchronises). */
int caro_dump_tree(caro_engine* h, int game, int store, int64_t cap, uint64_t* keys_dev, int32_t* N_dev,
                   float* W_dev, float* Q_dev, float* P_dev, int32_t* strong_dev, int64_t* n_nodes, void* stream);

/* ---- fused float32 policy/value net (lib/model.py:10-94, Net.forward in eval mode + F.softmax of
 *      lib/mcts.py:216) for the leaf batch.  Weights: one flat float32 host buffer in the order
 *      conv_in [9 taps][2][64], b[64]; K x 9 tap chunks of 4096 floats in the kernel's LDS image order
 *      (caro_ai_amd/net_hip.py packs them, batch-norm folded), b[K][64]; heads [3][64], b[3];
 *      value.0 [20][HW], b[20]; value.2 [20], b[1]; policy.0 [A][2HW], b[A].
 *      K = the number of residual blocks ("depth"): 5 (the reference's Net) through the calls without a depth
 *      argument, 1 .. caro_net_max_depth() through the *_depth calls.  Every layer of a net of any depth runs the
 *      arithmetic of the depth-5 kernels in their order; only the layer and weight-chunk counts follow K. ---- */
typedef struct caro_net caro_net;
int64_t caro_net_packed_size(int H, int W, int A);
int caro_net_create(int H, int W, int A, float negative_slope, const float* packed_host, int64_t n_floats,
                    int device_id, caro_net** out);
/* caro_net_packed_size / caro_net_create for a residual tower of `depth` blocks (depth 5 = those calls, and the same
 * kernels; any other depth runs the run-time-depth instantiation of the same kernel code).  depth < 1 or
 * > caro_net_max_depth(), or a buffer that is not caro_net_packed_size_depth(H, W, A, depth) floats: CARO_E_INVAL (the
 * size functions return it in place of a size).  Argument checks come first, CARO_E_NODEV after them, as in
 * caro_net_create. */
int caro_net_max_depth(void);
int64_t caro_net_packed_size_depth(int H, int W, int A, int depth);
int caro_net_create_depth(int H, int W, int A, int depth, float negative_slope, const float* packed_host,
                          int64_t n_floats, int device_id, caro_net** out);
/* residual blocks of a conv net (0 for NULL and for the table evaluator, which has no depth) */
int caro_net_depth(const caro_net* n);
/* f32w mode: the 3x3 convolutions in row-Winograd F(2,3) form (float32 MFMA, two thirds of the multiplies;
 * results differ from the direct form by float32 rounding only).  ww_host = [K][4][3][4096] floats, K = the net's
 * depth (caro_net_winograd_size_depth(K) of them), from caro_ai_amd/net_hip.py:pack_net_w ([layer][transformed tap p]
 * [dx], each in the order of the plain tap chunks); the library re-orders them into the chunks its kernel streams
 * ([layer][dx][granule half][p]) at upload.  Lowers caro_net_boards_per_workgroup if 128 / (ceil(H/2)*W) is smaller.
 * An image sized for another depth is CARO_E_INVAL (likewise in the two enable calls below). */
int64_t caro_net_winograd_size_depth(int depth);
int caro_net_enable_winograd(caro_net* n, const float* ww_host, int64_t n_floats);
/* f32w2 mode for LARGE boards (one board per workgroup: 12x12 .. 15x15): the 3x3 convolutions of lib/model.py:36-47 in
 * 2-D Winograd F(2x2,3x3) form -- 16 / 36 of the direct form's multiplies (the row form of caro_net_enable_winograd:
 * 24 / 36), the same float32 network function within the tolerance of tests/test_gpu_net.py.  ww2_host: the transformed
 * weights in kernel order, caro_net_winograd2d_size() floats (caro_ai_amd/net_hip.py:pack_net_w2).  Mutually exclusive
 * with the other arithmetic modes of a net.  A forward call of such a net is TWO launches on the caller's stream: the
 * trunk (one board per workgroup) and the FC heads + softmax of the whole call, 32 boards per workgroup; the first call
 * allocates the feature rows that travel between them (3 * H * W floats per row of the largest launch seen).  The rows
 * are kept per (net handle, stream) -- the first net's, for a pair -- so launches of one handle on different streams may
 * overlap; a handle serves at most 8 streams, and host calls on one handle are not thread-safe. */
int caro_net_winograd2d_size(void);
/* caro_net_winograd2d_size for a net of `depth` residual blocks ([depth][8 chunks] of 8192 floats) */
int64_t caro_net_winograd2d_size_depth(int depth);
int caro_net_winograd2d_supported(int H, int W);
int caro_net_enable_winograd2d(caro_net* n, const float* ww2_host, int64_t n_floats);
/* bf16x3 mode -- an EXTRA arithmetic mode, not the default of any caller and not what bench.py's headline runs: every
 * float32 operand of the residual trunk (lib/model.py:36-47) as the sum of three bfloat16 parts, a product as the six
 * part products of weight 2^-16 and above on v_mfma_f32_16x16x32_bf16, float32 accumulation; conv_in, biases, residual
 * adds, LeakyReLU and the heads in float32 as in the default kernel.  NOT bit-identical to the float32 modes: within
 * the tolerance tests/test_gpu_net.py states for it.  parts_host: caro_net_split_bf16_size() uint16 =
 * [45 (layer, tap)][2 c][3 parts][4 kg][64 co][8 ci] bfloat16 bit patterns, ci = 32 c + 8 kg + 0..7
 * (caro_ai_amd/net_hip.py:pack_net_x3).  Mutually exclusive with the other arithmetic modes of a net.  On boards served one
 * per workgroup (12x12 .. 15x15) a forward call is two launches, as in f32w2 mode: the trunk, then the FC heads + softmax of
 * the whole call 32 boards per workgroup, with the feature rows kept per (net handle, stream) as described below. */
int64_t caro_net_split_bf16_size(void);
/* caro_net_split_bf16_size for `depth` residual blocks: what caro_ai_amd/net_hip.py:pack_net_x3 returns for such a net.
 * The bf16x3 KERNEL is built for depth 5 only: caro_net_enable_split_bf16 on a net of any other depth is CARO_E_INVAL
 * ("bf16x3 form: built for nets of 5 residual blocks only ..."), never a fall-back to another form. */
int64_t caro_net_split_bf16_size_depth(int depth);
int caro_net_enable_split_bf16(caro_net* n, const uint16_t* parts_host, int64_t n_u16);
/* how often a slot of that (handle, stream) table had to change its stream: 0 while a handle serves at most 8 streams;
 * every eviction costs a device synchronisation (the slot's rows are re-used, not re-allocated) */
int64_t caro_net_stream_evictions(const caro_net* n);
void caro_net_destroy(caro_net* n);
int caro_net_boards_per_workgroup(const caro_net* n);
/* Two forms of the row-Winograd kernel (caro_net_enable_winograd): the general one serves every board, one net or two;
 * the fixed-shape one has connect four's shape (6 x 7, 7 actions, tiles of 6 / 3 / 1 boards) as compile-time constants
 * and takes one net.  A launch runs the fixed-shape form iff the net is in the row-Winograd mode, has the reference's
 * depth and connect four's shape, and the launch is of one net (caro_net_forward, caro_net_forward_slots with n1 ==
 * NULL); both forms return the same bits.
 * caro_net_set_kernel_form: form 0 = automatic (the default), 1 = always the general form; anything else is
 *   CARO_E_INVAL.  CARO_NET_KERNEL_FORM=1 in the environment when the library is loaded makes 1 the start value of every
 *   net (A/B runs of an unchanged program).
 * caro_net_kernel_form: 0 (fixed shape) or 1 (general), what the next one-net launch of this net would run.
 * caro_net_last_launch_form: the same for the last launch that went through this handle as n0, a two-net launch
 *   included (always 1); -1 before the first launch of a row-Winograd net. */
int caro_net_set_kernel_form(caro_net* n, int form);
int caro_net_kernel_form(const caro_net* n);
int caro_net_last_launch_form(const caro_net* n);
/* 1 if the net's kernel reads the slot_list_dev of caro_net_forward_slot_list (the one-board-per-workgroup 2-D Winograd
 * form), 0 if it ignores it: the engine's multi-wave tree kernels write the list only then */
int caro_net_uses_slot_list(const caro_net* n);
/* rows [row0, row0 + L) of planes_dev f32[max_rows,2,H,W] -> probs_dev f32[.,A] (softmaxed), values_dev f32[.]
 * with L = counts_dev[which] and row0 = which ? counts_dev[0] : 0, both read ON DEVICE. */
int caro_net_forward(caro_net* n, const float* planes_dev, const int32_t* counts_dev, int which, int64_t max_rows,
                     float* probs_dev, float* values_dev, void* stream);

/* slot rows, the form the fused tree kernel of caro_search_batch produces: the j-th unique leaf of game g sits
 * at row g * batch + j of planes_dev (its priors / value come back in the same row of probs_dev / values_dev),
 * gpack_dev i32[n_games] = leaf count | net class << 8, counts_dev = {L0, L1} totals per net, all read ON DEVICE.
 * Every workgroup maps its dense tile of boards onto the slot rows in game order itself, so which leaves share a
 * tile (and the tile size) is a function of the games' states only, never of block arrival order.
 * n1 may be NULL (one net, every game class 0). */
int caro_net_forward_slots(caro_net* n0, caro_net* n1, const float* planes_dev, const int32_t* counts_dev,
                           const int32_t* gpack_dev, int n_games, int batch, float* probs_dev, float* values_dev,
                           void* stream);

/* The same with the dense order of the leaves GIVEN by the producer: slot_list_dev i32[2][n_games * batch], entry
 * [c][i] = slot row of the i-th leaf of net class c (i < counts_dev[c]), in any order -- the multi-wave fused tree kernel
 * of caro_search_batch appends a game's rows when its block gets there.  Only the net forms that serve ONE board per
 * workgroup use it (2-D Winograd, 12x12 .. 15x15: a board's arithmetic does not depend on its dense index, and no
 * workgroup has to derive the map from gpack_dev any more); every other form ignores the list and keeps the game-order
 * map, so which boards share a tile stays a function of the games' states.  slot_list_dev may be NULL. */
int caro_net_forward_slot_list(caro_net* n0, caro_net* n1, const float* planes_dev, const int32_t* counts_dev,
                               const int32_t* gpack_dev, const int32_t* slot_list_dev, int n_games, int batch,
                               float* probs_dev, float* values_dev, void* stream);

/* Table evaluator with the same launch interface as the conv net (leaf counts read on device, dense or slot
 * rows): an exact integer-hash "net" for checking the SEARCH bit for bit -- it stands where lib/mcts.py:212-218
 * calls the net.  With x = the 2*H*W input planes of a row, mix64 = the splitmix64 finaliser of caro_noise.h:
 *   h    = salt + sum over j with x[j] != 0 of (mix64(0x5851f42d4c957f2d + j) | 1)          (mod 2^64)
 *   P[a] = (((mix64(h + 0x9E3779B97F4A7C15 * (a + 1)) >> 20) & 1023) + 1) / 8192            (float32, exact)
 *   v    = ((mix64(h ^ 0xA5A5A5A5A5A5A5A5) >> 20) % 2001 - 1000) / 1024                      (float32, exact)
 * (P is used as is, no softmax).  oracle/caro_oracle.c and tests/synth_net.py hold independent twins.
 *
 * Those values are multiples of 2^-13 / 2^-10, so every float32 sum the search forms from them is exact in ANY order.
 * Grain 1 is the same evaluator (h as above) with full-mantissa values, under which a float32 running sum such as W
 * depends on the order of its terms:
 *   P[a] = (((mix64(h + 0x9E3779B97F4A7C15 * (a + 1)) >> 20) & 0xFFFFFF) + 1) / 2^27        (integer <= 2^24: exact)
 *   v    = ((mix64(h ^ 0xA5A5A5A5A5A5A5A5) >> 20) % 33554431 - 16777215) / 2^24              (|integer| < 2^24: exact)
 * caro_net_create_hash is grain 0; any grain but 0 or 1 is CARO_E_INVAL; the two nets of a pair launch share one grain. */
int caro_net_create_hash(int H, int W, int A, uint64_t salt, int device_id, caro_net** out);
int caro_net_create_hash_grain(int H, int W, int A, uint64_t salt, int grain, int device_id, caro_net** out);

/* A HIP stream confined to the compute units [part/nparts, (part+1)/nparts) of the device
 * (hipExtStreamCreateWithCUMask): independent engines on such streams run side by side on disjoint CUs. */
int caro_stream_create_partition(int device_id, int part, int nparts, void** stream_out);
int caro_stream_destroy(void* stream);
/* both nets of an arena in ONE launch: rows [0, L0) through n0, rows [L0, L0+L1) through n1.  The nets must agree in
 * board shape, kind and arithmetic mode; they may differ in depth (each net's workgroups run its own tower). */
int caro_net_forward_pair(caro_net* n0, caro_net* n1, const float* planes_dev, const int32_t* counts_dev,
                          int64_t max_rows, float* probs_dev, float* values_dev, void* stream);
/* the same with n1's rows starting at row1_base instead of L0 (row1_base < 0: at L0) */
int caro_net_forward_pair_at(caro_net* n0, caro_net* n1, const float* planes_dev, const int32_t* counts_dev,
                             int64_t row1_base, int64_t max_rows, float* probs_dev, float* values_dev, void* stream);
/* diagnostic form: also writes per workgroup (total shader cycles, 100 MHz wall ticks, cycles at trunk start, at trunk end) to stamps_dev u64[4*grid],
 * grid = ceil(max_rows / caro_net_boards_per_workgroup); used by tools/probe_clock.py only */
int caro_net_forward_stamped(caro_net* n, const float* planes_dev, const int32_t* counts_dev, int which,
                             int64_t max_rows, float* probs_dev, float* values_dev, uint64_t* stamps_dev,
                             void* stream);
/* diagnostic: from now on every launch of this net's float32 kernels -- the engine's own launches included -- writes the
 * same per-workgroup stamps to stamps_dev u64[4 * grid] (grid <= games * batch / boards per workgroup + 2);
 * NULL switches it off.  tools/probe_engine_net.py only */
int caro_net_debug_stamps(caro_net* n, uint64_t* stamps_dev);
/* MCTS.search_batch (lib/mcts.py:162-176) for every live game with the fused net(s): `searches` x
 * (caro_select -> caro_net_forward per net -> caro_expand_backup) enqueued on `stream` from one call, no host
 * synchronisation.  noise_dev: f64[searches, G, batch, A] or NULL (generated); buffers as for caro_select /
 * caro_expand_backup (G * batch rows); net1 may be NULL when the engine has one net.  With one wavefront per game
 * (batch * lanes-per-descent == 64) the three tree kernels run fused (k_tree), two launches per minibatch, and
 * leaves travel in slot rows (caro_net_forward_slots); with several whole wavefronts per game (a multiple of 64 above
 * 64) the same fusion runs as k_tree_mw; otherwise (less than one wavefront) in the dense rows of caro_select.
 * A move needs searches >= 2 when its root may be unexpanded: the first minibatch on an unexpanded root only expands it
 * (lib/mcts.py:123: every descent returns the root itself, nothing is backed up), so after ONE search no edge has been
 * visited and the policy is 0 / 0 -- the reference raises ZeroDivisionError there (lib/mcts.py:311); caro_policy
 * returns NaN rows for such a game, and caro_step / the staggered ply REFUSE the ply (the game stays where it was,
 * actions_dev = -1, counters[5] is bumped) when tau = 1 or when action 0 -- the reference's argmax of an all-zero
 * row at tau = 0 -- is not a legal move. */
int caro_search_batch(caro_engine* h, caro_net* net0, caro_net* net1, int searches, int batch,
                      const double* noise_dev, float* planes_dev, uint64_t* leaf_keys_dev, float* probs_dev,
                      float* values_dev, void* stream);

/* One whole move of play_game's loop body (lib/utils.py:76-99: search_batch, get_policy_value, the sampled move,
 * game.move, win / draw) for every live game: caro_search_batch followed by caro_step, arguments as for those two.
 * Where several wavefronts serve a game (batch x lanes per descent a multiple of 64 above 64: the 15 x 15 board with 8
 * descents) the ply -- and, with caro_config.evict, the eviction that follows it -- runs inside the search's closing
 * tree launch: one launch per move instead of three.  Results are those of the two calls. */
int caro_search_move(caro_engine* h, caro_net* net0, caro_net* net1, int searches, int batch, const double* noise_dev,
                     const double* uniforms_dev, float* planes_dev, uint64_t* leaf_keys_dev, float* probs_dev,
                     float* values_dev, int32_t* actions_dev, int32_t* done_dev, int32_t* result_dev, void* stream);

/* ---- staggered mode: every game on its own minibatch clock (the hot path of bench.py / train.self_play) ----
 * In lock-step all games reach a move together, and the launches right after a move carry far more new leaves
 * than the rest, so the net launch overflows one round of tiles exactly there.  The reference plays its games one
 * after another (train.py:41-47) -- nothing ties their moves together -- so here each game counts its own
 * minibatches: game g sits out g % searches launches at the start, makes its ply INSIDE the tree kernel when its
 * `searches` minibatches are done (lib/utils.py:80-99), and a finished game is parked (record + history rows copied
 * aside) and its slot restarted at once (uid += uid_stride) when `recycle` != 0.  Every launch then carries the
 * same mix of minibatch indices.  Game by game the results are those of caro_search_batch + caro_step: the same
 * minibatches on the same tree with the same noise keys.  Needs whole wavefronts per game (batch x lanes per descent a
 * multiple of 64: connect four with batch 8 = one wavefront, k_tree_stag; several wavefronts -- TicTacToe with batch 8,
 * 15 x 15 with batch 8 -- k_tree_stag_mw, round 6), generated noise / move uniforms, a fresh or restarted engine.
 * caro_config.evict combines with it where several wavefronts serve a game: the eviction then runs inside the kernel,
 * right behind the game's ply (a finished game drops every node, which also leaves both key tables clean for the restart).
 *   caro_config.stagger     = mcts_searches at caro_engine_create (fixed for the engine's life)
 *   caro_search_staggered   `launches` x (tree kernel -> net kernel); on average every game moves once per
 *                           `searches` launches
 *   caro_drain_parked_begin tuples of the parked games, as caro_drain_tuples_begin (no recycle flag: the slots have
 *                           restarted already); finish with caro_drain_tuples_end
 * A staggered engine is driven by these two calls only: the lock-step mutators (caro_reset_games, caro_set_roots,
 * caro_select, caro_search_batch, caro_step, caro_drain_tuples[_begin]) return CARO_E_STATE on it -- they know nothing
 * of its per-game clocks, pending minibatches and parked records.  Read-only calls (caro_counters, caro_get_roots,
 * caro_policy, caro_lookup_nodes, caro_tree_sizes, caro_pending_leaves ...) work on both kinds. */
int caro_search_staggered(caro_engine* h, caro_net* net0, caro_net* net1, int launches, int batch, float* planes_dev,
                          uint64_t* leaf_keys_dev, float* probs_dev, float* values_dev, void* stream);
int caro_drain_parked_begin(caro_engine* h, int64_t cap, uint64_t* states_dev, int32_t* players_dev, double* pi_dev,
                            int32_t* z_dev, int64_t* games_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CARO_HIP_H */
