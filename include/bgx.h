/*
 * bgx.h — C ABI of the MI355X-native backgammon self-play engine (libbgx.so).
 *
 * Plain C: pointers and sizes only, no exceptions, no torch/HIP types.  Every
 * device pointer is a HIP device allocation on the engine's device; `stream`
 * is a hipStream_t passed as void* (NULL = the default stream).  All work is
 * enqueued on that stream; no entry point synchronises the host unless it says
 * so.  Return value: BGX_OK (0) or a negative bgx_status.
 *
 * Each entry point names the reference interface it replaces
 * (Nick-qsv/MLP-PPO-2PLY-P3, paths relative to its src/).
 *
 * Data formats
 *   board52   int8[52]  = P1 points[24], P2 points[24], bar[2] (P1,P2), off[2]
 *                         (the reference's (4,24) int8 tensor, immutable_board.py:20-24,
 *                          with its 44 always-zero bytes dropped)
 *   move      uint64    = up to 4 sub-moves, sub-move i in bits 16i..16i+15:
 *                         start(5) | end(5)<<5 | hits_blot(1)<<10 | valid(1)<<15,
 *                         start/end are Position values (0..23, BAR=24, BEAR_OFF=25)
 *                         (SubMove/FullMove, moves/move_types.py:38-48)
 *   features  float[198] per board (immutable_board.py:171-212)
 *   info      int32 per lane: mover | (winner+1)<<8 | game_score<<16 | kind<<24,
 *                         kind 0 = move, 1 = pass, 2 = invalid action, 3 = reset on game over
 */
#ifndef BGX_H
#define BGX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bgx_engine bgx_engine;

enum bgx_status {
    BGX_OK = 0,
    BGX_EINVAL = -1,     /* bad argument */
    BGX_EDEVICE = -2,    /* HIP error (launch, memory, device selection) */
    BGX_ENOMEM = -3,     /* device allocation failed */
    BGX_EOVERFLOW = -4,  /* a position exceeded the slow-path dedup capacity */
    BGX_ESTATE = -5      /* the engine's lanes changed while a call was reading them (see below) */
};

/* Stream ordering.  Every call that takes a bgx_engine* orders itself after the
 * engine's previous call: when it comes on a different stream than that call, its
 * stream first waits (hipStreamWaitEvent) for the previous call's work, so a step on
 * one stream followed by bgx_two_ply / bgx_one_ply / bgx_copy_lanes / ... on another
 * reads the lanes the step wrote (the engine's lanes, move lists, overflow queues and
 * tables and the search workspace are one piece of device state).  Calls captured into
 * a HIP graph are ordered by the graph: its launch stream must follow whatever else
 * used the engine, and a call after a graph launch on another stream must be ordered
 * by the caller.  Kernels that take raw lane pointers (bgx_policy_act*, reading
 * bgx_buffers.lanes) run on the caller's stream as given.  The host-side state calls
 * without a stream (bgx_engine_seed, bgx_engine_mt_state, bgx_engine_error) synchronise
 * the device before and after.  bgx_two_ply returns
 * BGX_ESTATE (and bgx_one_ply sets bit 1 of the engine's error word) if it finds a
 * lane whose legal moves no longer match its row layout, instead of reading past them. */

enum bgx_dice_mode {
    BGX_DICE_MT_LANE = 0,    /* lane i == one BackgammonEnv after env.seed(seeds[i]) (numpy legacy MT19937) */
    BGX_DICE_MT_SHARED = 1,  /* one numpy stream consumed in lane order == VectorizedBackgammonEnv after np.random.seed */
    BGX_DICE_PHILOX = 2      /* Philox4x32-10 per lane (speed mode; same die distribution) */
};

/* BackgammonEnv(match_length, max_legal_moves) x batch (backgammon_env.py:38-75,
 * vec_bg_env.py:8-18).  auto_reset=1: a finished game is reset inside the same
 * step and the post-reset observation is returned (VectorizedBackgammonEnv.step,
 * vec_bg_env.py:35-36); auto_reset=0: BackgammonEnv semantics (the NEXT step
 * resets and returns done=1, backgammon_env.py:119-121). */
int bgx_engine_create(int device, int32_t batch, int32_t max_moves, uint64_t seed, int32_t dice_mode,
                      int32_t auto_reset, int32_t match_length, bgx_engine** out);
/* Order `stream` after every piece of a step still running on the engine's own
 * side streams (the next step's order pass): a HIP graph capture of steps
 * calls it before capturing and as its last captured call, so the graph holds no
 * work it does not join. */
int bgx_engine_join(bgx_engine* e, void* stream);
/* Test accessor of the dispatch order (Philox engines; never on a step's path): joins a
 * pending order pass into `stream`, copies the order perm (int32[batch], launch position ->
 * lane) the next step will use, the resolved cost classes (uint8[batch], 0 = heaviest .. 4)
 * and the Philox counters with their roll-cache bits (uint64[batch]) to HOST buffers, and
 * synchronises the stream.  A step or reset leaves the classes; the order itself is laid
 * out at the start of the next bgx_step (with that step's actions), so for perm the call
 * runs that pass's perm-only form on `stream` -- the next step computes the same either way.  Any pointer may be NULL.  BGX_EINVAL for perm / classes when the engine
 * has no order (MT dice, BGX_ORDER 0) or has not built one yet (before the first reset). */
int bgx_engine_order(bgx_engine* e, int32_t* perm_host, uint8_t* cls_host, uint64_t* ctr_host, void* stream);
/* Where a Philox step's light launch (the non-predicted-doubles rest of the dispatch
 * order) and the next step's order pass (classes and counts) run: fork = 1 (default) on the engine's
 * side stream, fork-joined on events beside the heavy launch; fork = 0 on the caller's
 * stream after it.  Same results either way.  A HIP graph of fork = 0 steps is one
 * linear chain: several such engines on their own streams then map one-to-one onto
 * the hardware queues (bench.py C3: 4 shards), where forked graphs' internal streams
 * share queues with the other shards' and serialise them.
 * Turning the fork off joins a pending order pass into `stream`. */
int bgx_engine_set_fork(bgx_engine* e, int32_t fork, void* stream);
int bgx_engine_destroy(bgx_engine* e);

/* BackgammonEnv.seed (backgammon_env.py:357-363): per-lane MT19937 seeds
 * (host array of `batch` uint32; mode SHARED uses seeds[0]); Philox: key = seed. */
int bgx_engine_seed(bgx_engine* e, const uint32_t* seeds_host, uint64_t philox_seed);

/* Read (set=0) or overwrite (set=1) the MT19937 state of one lane (mode
 * MT_LANE) or of the shared stream (mode MT_SHARED, lane ignored):
 * state_host uint32[625] = numpy's get_state() key[624] + pos.  Lets the
 * drop-in classes draw dice from numpy's global RandomState exactly as the
 * reference does (backgammon_env.py:245-246).  Synchronous. */
int bgx_engine_mt_state(bgx_engine* e, int32_t lane, uint32_t* state_host, int32_t set);

/* Device buffers owned by the engine (read-only for callers unless stated). */
typedef struct {
    uint8_t* lanes;      /* [batch][64] lane records: board52, cur(52), roll(53,54), game_over(55),
                            match_over(56), score P1/P2 (57,58), n_moves int16 (60,61) */
    uint64_t* moves;     /* [batch][max_moves] legal moves of the current position */
    int32_t* n_total;    /* [batch] untruncated legal-move count (len before [:max_moves]) */
    int32_t batch, max_moves;
} bgx_buffers;
int bgx_engine_buffers(bgx_engine* e, bgx_buffers* out);

/* BackgammonEnv.reset (backgammon_env.py:78-113) for lanes with lane_mask[i]!=0
 * (lane_mask NULL = all lanes).  obs_dev: float[batch][198] (all lanes written; may be NULL). */
int bgx_reset(bgx_engine* e, const uint8_t* lane_mask_dev, float* obs_dev, void* stream);

/* BackgammonEnv.step / VectorizedBackgammonEnv.step (backgammon_env.py:115-191,
 * vec_bg_env.py:28-49) on every lane.  actions_dev int32[batch]; outputs
 * obs float[batch][198], reward float[batch], done uint8[batch], info int32[batch]
 * (obs_dev and info_dev may be NULL: a rollout that stores int8 boards skips the
 * 792-byte fp32 observation). */
int bgx_step(bgx_engine* e, const int32_t* actions_dev, float* obs_dev, float* reward_dev, uint8_t* done_dev,
             int32_t* info_dev, void* stream);

/* get_all_possible_moves (moves/get_all_moves.py:9-70) + truncation to max_moves
 * (backgammon_env.py:219-231) on n arbitrary positions.  boards52_dev int8[n][52],
 * players_dev uint8[n], dice_dev uint8[n][2]; outputs n_moves int16[n] (truncated),
 * n_total int32[n] (untruncated, may be NULL), moves uint64[n][max_moves]. */
int bgx_movegen(bgx_engine* e, const int8_t* boards52_dev, const uint8_t* players_dev, const uint8_t* dice_dev,
                int32_t n, int32_t max_moves, int16_t* n_moves_dev, int32_t* n_total_dev, uint64_t* moves_dev,
                void* stream);

/* ImmutableBoard.get_board_features (immutable_board.py:171-212) /
 * get_board_features_batch_from_tensors (ai/batching.py:78-147). */
int bgx_encode(const int8_t* boards52_dev, const uint8_t* players_dev, int32_t n, float* out_dev, void* stream);

/* The same 198 features from n 64-byte lane records (records_dev: n x 64 bytes,
 * board bytes 0..51, player to move at byte 52 -- the rollout rows the PPO update
 * re-encodes, ppo_agent.py:221-229 / 274 stacks the stored observations and casts
 * them under autocast).  dtype 0: fp32 [n][198]; 1: fp16 [n][198], the round to
 * nearest of the fp32 features (autocast's cast). */
int bgx_encode_records(const uint8_t* records_dev, int32_t n, int32_t dtype, void* out_dev, void* stream);
/* The same with a row width of 198 or 208 elements: columns 198..width-1 are
 * zero (208: 16-byte aligned rows, which hipBLASLt's vector-load GEMMs need for
 * the PPO update's fc1 forward and weight gradient; the zero columns meet zero
 * weight columns, so the products are unchanged). */
int bgx_encode_records_ex(const uint8_t* records_dev, int32_t n, int32_t dtype, int32_t width, void* out_dev,
                          void* stream);

/* execute_full_move_on_board_copy (immutable_board.py:224-233) over every legal
 * move of lanes [lane0, lane0+nlanes): boards52 int8[nlanes][max_moves][52]
 * (rows past n_moves are zero). */
int bgx_afterstates(bgx_engine* e, int32_t lane0, int32_t nlanes, int8_t* boards52_dev, void* stream);

/* generate_all_board_features + zero padding (ai/batching.py:10-75,
 * backgammon_env.py:207-243) for lanes [lane0, lane0+nlanes):
 * out float[nlanes][max_moves][198], the mover's one-hot. */
int bgx_legal_features(bgx_engine* e, int32_t lane0, int32_t nlanes, float* out_dev, void* stream);

/* BackgammonEnv.action_mask / VectorizedBackgammonEnv.get_action_masks
 * (backgammon_env.py:232-236, vec_bg_env.py:51-56): counts_dev int16[batch]
 * (= number of legal actions, mask = iota < count; may be NULL) and/or
 * masks_dev float[batch][max_moves] (1.0 for the first count entries; may be NULL). */
int bgx_action_masks(bgx_engine* e, int16_t* counts_dev, float* masks_dev, void* stream);

/* Copy lane state [lane0, lane0+n) out of the engine (device-to-device, async):
 * lanes_dst uint8[n][64], moves_dst uint64[n][max_moves], n_total_dst int32[n];
 * any destination may be NULL.  (The reference exposes env.board / env.legal_moves
 * / env.current_player / env.roll_result as attributes, backgammon_env.py:51-75.) */
int bgx_copy_lanes(bgx_engine* e, int32_t lane0, int32_t n, uint8_t* lanes_dst, uint64_t* moves_dst,
                   int32_t* n_total_dst, void* stream);

/* Overwrite lane records [lane0, lane0+n) (board52 + metadata, 64 bytes each) and
 * re-enumerate their legal moves for the stored player/roll: lets a caller pose
 * arbitrary positions (tests, analysis).  lanes_src uint8[n][64] on the device. */
int bgx_set_lanes(bgx_engine* e, int32_t lane0, int32_t n, const uint8_t* lanes_src, void* stream);
/* bgx_set_lanes with regen = 0: the records are written as given and the stored
 * legal moves / counts are left as they were -- the reference's BackgammonEnv.roll_dice
 * and pass_turn change roll_result / current_player without touching legal_moves
 * until update_legal_moves() runs (backgammon_env.py:198-251); regen = 1 is
 * bgx_set_lanes (that update_legal_moves). */
int bgx_set_lanes_ex(bgx_engine* e, int32_t lane0, int32_t n, const uint8_t* lanes_src, int32_t regen, void* stream);

/* Rollout rows to pinned host memory (the reference keeps its rollout memory on
 * the host, ppo_agent.py:175-187): up to BGX_MAX_COPY_REGIONS strided 2-D copies in
 * ONE kernel launch, so a HIP graph of rollout steps can carry the copy of a slot
 * pair of every field as one node.  Region i copies `rows` rows of `width` bytes
 * from src (row pitch spitch) to dst (pitch dpitch); device pointers on both sides
 * (a pinned host buffer's device pointer from bgx_host_device_ptr); widths,
 * pitches and pointers 16-byte aligned.  workgroups <= 0: up to 64. */
#define BGX_MAX_COPY_REGIONS 8
typedef struct {
    const void* src;
    void* dst;
    int64_t width, rows, spitch, dpitch;
} bgx_region;
int bgx_copy_regions(const bgx_region* regions, int32_t n, int32_t workgroups, void* stream);
/* The device-side address of pinned (hipHostMalloc / torch pin_memory) host memory. */
int bgx_host_device_ptr(void* host_ptr, void** dev_ptr_out);

/* Sticky device error word (bit 0: a position overflowed the slow-path dedup
 * table; bit 1: bgx_one_ply found a lane changed under it, see "Stream ordering";
 * bit 2: bgx_engine_set_starts found an invalid start record).
 * Synchronises the engine's device. */
int bgx_engine_error(bgx_engine* e, int32_t* err_out);

/* ---- policy network (agent/policy_network.py:44-75) + select_action (ppo_agent.py:138-191) ----
 * Weights are packed once per update into MFMA operand order (f16 hi/lo split
 * pairs with power-of-two scales; fp32-equivalent results, see bg_mlp.hip):
 * bgx_policy_packed_size(H, A) floats; H <= 128.  Inputs are torch nn.Linear
 * layouts: W1 [H][198], b1 [H], Wa [A][H], ba [A], wv [H], bv [1]. */
int bgx_policy_packed_size(int32_t hidden, int32_t n_actions);
int bgx_policy_pack(const float* W1, const float* b1, const float* Wa, const float* ba, const float* wv, const float* bv,
                    int32_t hidden, int32_t n_actions, float* packed_dev, void* stream);

/* One fused pass per game lane: features from the 64-byte lane record
 * (bgx_buffers.lanes layout), relu(W1 x + b1), logits = Wa h + ba, value = wv h + bv,
 * masked = logits + log(mask + 1e-45) with mask = [a < legal count], then
 * action ~ Categorical(softmax(masked)) (Gumbel-max, noise hashed from (seed, step, row, a))
 * or argmax if greedy (eval mode, ppo_agent.py:188-191).  act_out int32[n],
 * logp_out float[n] (log softmax(masked)[action]), value_out float[n];
 * logits_out float[n][32*ceil((A+1)/32)] (raw logits, value at column A) may be
 * NULL, as may logp_out/value_out. */
int bgx_policy_act(const uint8_t* records_dev, int32_t n, const float* packed_dev, int32_t hidden, int32_t n_actions,
                   uint64_t seed, uint32_t step, int32_t greedy, int32_t* act_out, float* logp_out, float* value_out,
                   float* logits_out, void* stream);

/* bgx_policy_act that also writes each row's 64-byte input record to
 * records_out uint8[n][64] (the rollout's stored observation,
 * select_action appends the state to memory, ppo_agent.py:176-185), so a rollout reads the
 * engine's lane buffer (bgx_buffers.lanes) in place with no separate copy.
 * records_out may be NULL (then identical to bgx_policy_act). */
int bgx_policy_act_rec(const uint8_t* records_dev, int32_t n, const float* packed_dev, int32_t hidden,
                       int32_t n_actions, uint64_t seed, uint32_t step, int32_t greedy, int32_t* act_out,
                       float* logp_out, float* value_out, float* logits_out, uint8_t* records_out, void* stream);

/* bgx_policy_act_rec whose noise step is step + *step_ctr, read on the device when
 * the kernel runs (step_ctr may be NULL: then exactly bgx_policy_act_rec).  A HIP
 * graph that captures rollout steps replays with fresh draws when the graph also
 * advances the counter (bgx_counter_add). */
int bgx_policy_act_ctr(const uint8_t* records_dev, int32_t n, const float* packed_dev, int32_t hidden,
                       int32_t n_actions, uint64_t seed, uint32_t step, const uint32_t* step_ctr, int32_t greedy,
                       int32_t* act_out, float* logp_out, float* value_out, float* logits_out, uint8_t* records_out,
                       void* stream);
/* *ctr_dev += v on the stream (one thread). */
int bgx_counter_add(uint32_t* ctr_dev, uint32_t v, void* stream);

/* ---- value head search: V(x) = value_head(relu(fc1 x)), H <= 128 ----
 * bgx_value_pack packs fc1.weight [H][198], fc1.bias [H], value_head.weight [H],
 * value_head.bias [1] into bgx_value_packed_size(H) floats (MFMA operand order);
 * value_bias is value_head.bias[0] passed by value. */
int bgx_value_packed_size(int32_t hidden);
int bgx_value_pack(const float* W1, const float* b1, const float* wv, const float* bv, int32_t hidden,
                   float* packed_dev, void* stream);

/* 1-ply greedy over every lane's legal afterstates (features with the mover's
 * one-hot, as legal_board_features, backgammon_env.py:207-216): best_out int32[B]
 * = first argmax V, bestv_out float[B], values_out float[B][max_moves] (may be NULL). */
int bgx_one_ply(bgx_engine* e, const float* vpacked_dev, int32_t hidden, float value_bias, int32_t* best_out,
                float* bestv_out, float* values_out, void* stream);

/* 2-ply expectimax over the 21 rolls (get_all_dice_rolls.py:5-34) for every lane:
 * Q(a) = sum_r p_r min_{opponent replies b} V(enc(b, mover)), leaf = a when the
 * opponent cannot move (every leaf carries the root mover's one-hot, the
 * reference's evaluate_board(board, current_player), expect_minmax.py:57-58,
 * 100-143); best_out = first argmax Q.  q_out float[B][max_moves] and
 * bestq_out may be NULL; stats_host (may be NULL) receives {leaves evaluated,
 * (afterstate, roll) jobs, afterstates}.  Synchronises the stream (sizes its
 * workspace from the afterstate count). */
int bgx_two_ply(bgx_engine* e, const float* vpacked_dev, int32_t hidden, float value_bias, int32_t* best_out,
                float* bestq_out, float* q_out, uint64_t* stats_host, void* stream);

/* bgx_one_ply / bgx_two_ply for the lanes with lane_sel_dev[i] != 0 only (uint8[B] on the
 * device; NULL = every lane, which is exactly bgx_one_ply / bgx_two_ply).  An unselected
 * lane forms no rows (no afterstates, jobs or leaves: the work is that of the selected
 * lanes alone), its entries of best_out, bestv_out / bestq_out and values_out / q_out are
 * not written, stats_host counts the selected lanes only, and it is never reported as
 * changed (BGX_ESTATE / error bit 1).  Selected lanes get bit for bit what the unselected
 * call gives them.  An all-zero selection is legal: BGX_OK, nothing written, zero stats.
 * (The reference has one player act for every env, ppo_agent.py:138-191; a match between
 * two players needs each to act only where it is on move: bgx_arena_*.) */
int bgx_one_ply_sel(bgx_engine* e, const float* vpacked_dev, int32_t hidden, float value_bias,
                    const uint8_t* lane_sel_dev, int32_t* best_out, float* bestv_out, float* values_out,
                    void* stream);
int bgx_two_ply_sel(bgx_engine* e, const float* vpacked_dev, int32_t hidden, float value_bias,
                    const uint8_t* lane_sel_dev, int32_t* best_out, float* bestq_out, float* q_out,
                    uint64_t* stats_host, void* stream);

/* bgx_two_ply_sel behind a 1-ply move filter (DESIGN.md §5 "Move filter"; GNU Backgammon's
 * move filter, which the reference's commented-out expect_minmax.py lacks): the 1-ply value
 * V1(a) of every legal afterstate of the selected lanes (exactly bgx_one_ply_sel's values),
 * then per lane, on the order-preserving integer encoding of the float bits,
 *   rank(a) = #{b : V1(b) > V1(a)} + #{b < a : V1(b) == V1(a)}
 *   a is kept iff rank(a) < top_k and (rank(a) == 0 or V1(a) >= fp32(V1best - margin))
 * (margin = +inf: no threshold; margin = 0: the moves tied for best, top_k of them at most),
 * and the 2-ply search runs on the kept afterstates only.  best_out = the move index of the
 * first argmax of Q over the kept moves, bestq_out its Q; q_out[i][a] = Q(a) for a kept
 * move -- bit for bit its Q in the full search -- and -inf for a legal move that is not kept
 * (entries a >= n untouched); v1_out float[B][max_moves] (may be NULL) receives V1(a), a < n.
 * With top_k >= max_moves and margin = +inf, best_out, bestq_out and q_out are those of
 * bgx_two_ply_sel.  Unselected lanes: nothing is written; a lane without a legal move gets
 * what bgx_two_ply_sel gives it.  stats_host (uint64[4], may be NULL) receives {leaves
 * evaluated, (afterstate, roll) jobs, kept afterstates, candidate afterstates}.
 * BGX_EINVAL for top_k < 1, margin < 0 or NaN (nothing is written), and whatever
 * bgx_two_ply_sel rejects; BGX_ESTATE as there.  Synchronises the stream (sizes its
 * workspace from the kept afterstate count). */
int bgx_two_ply_topk(bgx_engine* e, const float* vpacked_dev, int32_t hidden, float value_bias,
                     const uint8_t* lane_sel_dev, int32_t top_k, float margin, int32_t* best_out,
                     float* bestq_out, float* q_out, float* v1_out, uint64_t* stats_host, void* stream);

/* The luck of each lane's roll (DESIGN.md §10 "Luck adjustment"; the variance reduction of
 * position rollouts, which the reference lacks).  Lane i holds board X, mover m (byte 52) and
 * the roll that was drawn (bytes 53, 54).  For each of the 21 rolls r in bgx_two_ply's order,
 *   v_r = max over m's legal afterstates b for r of V(enc(b, m))      (the mover's one-hot:
 *         bgx_one_ply's bestv for the lane (X, m, r)),   v_r = V(enc(X, m)) when m cannot move;
 *   mean = fma(p_20, v_20, ... fma(p_0, v_0, 0)) in fp32, p_r = 1/36 for doubles, else 2/36;
 *   luck = v_(the lane's own roll) - mean in fp32   (0 when bytes 53, 54 hold no roll).
 * vpacked_dev is the ordinary bgx_value_pack pack.  Lanes with lane_sel_dev[i] != 0 (NULL =
 * every lane) get luck_out[i] and, when it is given, mean_out[i] (float[B] each); the other
 * lanes' entries are not written.  stats_host (uint64[3], may be NULL) receives {leaves
 * evaluated, (lane, roll) jobs = 21 x rows, rows = selected lanes}.  An all-zero selection is
 * BGX_OK with zero stats.  BGX_EINVAL for a NULL engine, pack or luck_out, or hidden out of
 * range.  It reads the lane records only, not the stored move lists: no BGX_ESTATE case.
 * Ordered like every engine call.  Synchronises the stream (it sizes its workspace from the
 * selected-lane count and may run retry rounds, as bgx_two_ply does): not graph-capturable. */
int bgx_roll_luck(bgx_engine* e, const float* vpacked_dev, int32_t hidden, float value_bias,
                  const uint8_t* lane_sel_dev, float* luck_out, float* mean_out, uint64_t* stats_host, void* stream);

/* bgx_roll_luck's 21 values themselves (the cubeful luck needs them, as Janowski's
 * equity is piecewise linear in v): values_out float[B][21], values_out[i][r] = v_r above for the
 * 21 rolls r in bgx_two_ply's order, on the lanes with lane_sel_dev[i] != 0 (NULL = every lane);
 * the other lanes' rows are not written.  The fp32 FMA chain over a row is bgx_roll_luck's
 * mean_out[i] bit for bit, and v_(the lane's own roll) - mean its luck_out[i].  In every other
 * respect the contract is bgx_roll_luck's: ordering, the synchronisation, stats_host, an all-zero
 * selection, and BGX_EINVAL for a NULL engine, pack or values_out, or hidden out of range. */
int bgx_roll_values(bgx_engine* e, const float* vpacked_dev, int32_t hidden, float value_bias,
                    const uint8_t* lane_sel_dev, float* values_out, uint64_t* stats_host, void* stream);

/* The static value of lane records (the value a truncated rollout scores a game
 * with).  records_dev = uint8[n][64] lane records, 16-byte aligned (the engine's, or any copy);
 * vpacked_dev the ordinary bgx_value_pack pack, every hidden with bgx_value_packed_size >= 0.
 * For a lane with lane_sel_dev[i] != 0 (NULL = every lane):
 *   value_out[i] = wv . relu(W1 x + b1) + bv,   x = the 198 features of the record's board with
 *   the one-hot of the record's mover (byte 52): the x bgx_policy_act forms from the same record,
 *   and bgx_roll_luck's v_r of a mover that cannot move,
 * in the search kernels' fp32-equivalent (split-f16 MFMA) arithmetic; the roll bytes are not
 * read.  A lane's value does not depend on the selection: selected entries are bit for bit
 * those of the call with NULL.  Unselected lanes are not written; an all-zero selection is
 * BGX_OK.  A workgroup packs the selected lanes of its chunk of 256 or 512 lanes before it
 * evaluates them and stages the weights only once it meets a selected lane, so the cost follows
 * the chunks that hold one; no scratch is needed.  Runs on the caller's stream as given (no
 * engine, so no ordering of its own).  No allocation, no synchronisation, no host read:
 * graph-capturable (the first call per device and width asks the occupancy once; make it
 * outside a capture).  BGX_EINVAL for n <= 0, a NULL records, pack or value_out, records that
 * are not 16-byte aligned or hidden out of range. */
int bgx_value_lanes(const uint8_t* records_dev, int32_t n, const float* vpacked_dev, int32_t hidden,
                    float value_bias, const uint8_t* lane_sel_dev, float* value_out, void* stream);

/* ---- head-to-head arena (csrc/bg_engine.hip; bgx/arena.py) ----
 * Two players A and B play each other on the n lanes of an engine created with
 * auto_reset = 1 until every lane has finished games_per_lane games (the reference has no
 * evaluation match; its train.py:55-99 logs self-play statistics only).  The caller owns
 * the state, plain device arrays: games_done int32[n], sel_a / sel_b uint8[n] (the lanes
 * where A / B is on move now: the lane selection of bgx_one_ply_sel / bgx_two_ply_sel) and
 * tally int64[16] (indices below).  Seat rule: in game g of lane i, A is PLAYER1 iff
 * ((i + g) & 1) == 0.  A lane is active while games_done[i] < games_per_lane; afterwards it
 * belongs to neither player, is given action 0 and is not counted.  records_dev = the
 * engine's lane records (bgx_buffers.lanes), read in place on the caller's stream.  No
 * entry point synchronises or allocates: all three can be captured into a HIP graph.
 * bgx_arena_begin: games_done = 0, tally = 0, sel_a / sel_b from the lanes' movers,
 * tally[BGX_ARENA_ACTIVE] = number of active lanes.
 * bgx_arena_merge: actions[i] = sel_a[i] ? act_a[i] : sel_b[i] ? act_b[i] : 0.
 * bgx_arena_advance: after bgx_step, with that step's done and info.  Every lane that was
 * active in the step adds a ply; a done with a winner adds the game to the tally (winner
 * and game_score from info) and to games_done; sel_a / sel_b are set for the new position;
 * tally[BGX_ARENA_ACTIVE] drops by the lanes that finished their last game. */
enum bgx_arena_field {
    BGX_ARENA_GAMES = 0,          /* finished games */
    BGX_ARENA_WINS_A = 1,         BGX_ARENA_WINS_B = 2,
    BGX_ARENA_POINTS_A = 3,       BGX_ARENA_POINTS_B = 4,        /* 1 / 2 / 3 per game won */
    BGX_ARENA_GAMMONS_A = 5,      BGX_ARENA_GAMMONS_B = 6,
    BGX_ARENA_BACKGAMMONS_A = 7,  BGX_ARENA_BACKGAMMONS_B = 8,
    BGX_ARENA_GAMES_A_P1 = 9,     /* finished games in which A sat as PLAYER1 */
    BGX_ARENA_WINS_A_P1 = 10,     /* A's wins in those games */
    BGX_ARENA_WINS_P1 = 11,       /* wins by the PLAYER1 seat, whoever held it */
    BGX_ARENA_PLIES = 12,         /* steps of active lanes, passes included */
    BGX_ARENA_ACTIVE = 13         /* active lanes remaining; 14, 15 stay zero */
};
int bgx_arena_begin(const uint8_t* records_dev, int32_t n, int32_t games_per_lane, int32_t* games_done_dev,
                    uint8_t* sel_a_dev, uint8_t* sel_b_dev, int64_t* tally_dev, void* stream);
int bgx_arena_merge(const uint8_t* sel_a_dev, const uint8_t* sel_b_dev, const int32_t* act_a_dev,
                    const int32_t* act_b_dev, int32_t n, int32_t* actions_dev, void* stream);
int bgx_arena_advance(const uint8_t* records_dev, const uint8_t* done_dev, const int32_t* info_dev, int32_t n,
                      int32_t games_per_lane, int32_t* games_done_dev, uint8_t* sel_a_dev, uint8_t* sel_b_dev,
                      int64_t* tally_dev, void* stream);
/* A uniformly random legal action per lane record (the arena's baseline opponent; the
 * reference has no counterpart): act_out[i] =
 * floor(u * count_i), u in [0, 1) hashed from (seed, step, i), count_i = the record's legal
 * count (bytes 60-61); 0 when the lane has no legal move.  Graph-capturable. */
int bgx_random_act(const uint8_t* records_dev, int32_t n, uint64_t seed, uint32_t step, int32_t* act_out,
                   void* stream);

/* ---- start positions (no counterpart in the reference, whose env always resets to the
 * opening, backgammon_env.py:78-113) ----
 * starts_dev uint8[batch][64] in the lane-record layout (16-byte aligned), or NULL:
 * standard openings again.  The engine keeps a copy of its own; the call is ordered on
 * `stream` like every engine call and does not synchronise the host.  Lanes are not touched
 * by the call: the table takes effect at each lane's next reset, whichever path triggers it
 * (bgx_reset, masked or not; the auto-reset inside a step; the reset step of an
 * auto_reset = 0 engine).  A reset of lane i with a valid start record s: board (bytes
 * 0..51) and mover (byte 52) become s's, game_over 0, scores and the match flag as in the
 * standard reset.  The roll is s's bytes 53, 54 when both are in 1..6 (no die is drawn);
 * when both are 0 the lane draws two dice from its own stream as a mid-game roll does
 * (doubles allowed, no starter draw, no rejection).  Bytes 55..63 of s are ignored.
 * A record is valid when each side's points + bar + off == 15, no point is held by both
 * sides, both off counts are < 15, the mover is 0 or 1 and the roll is (0, 0) or two dice
 * in 1..6.  An invalid record sets bit 2 of the error word (bgx_engine_error) and its lane
 * resets to the standard opening.  BGX_EINVAL for a BGX_DICE_MT_SHARED engine (one stream
 * in lane order mirrors the reference's vector env, which has no start positions). */
int bgx_engine_set_starts(bgx_engine* e, const uint8_t* starts_dev, void* stream);

/* ---- position rollouts (csrc/bg_engine.hip; bgx/rollout.py; no counterpart in the
 * reference) ----
 * n lanes of an auto_reset = 1 engine whose start table is starts_dev play
 * games_per_lane games each from their start records, one player acting for both sides;
 * the results are tallied per position.  The caller owns the state, plain device arrays:
 * group int32[n] (lane -> position in [0, n_groups); any other value: an idle lane, never
 * selected, never counted, to be given action 0), games_done int32[n], plies int32[n]
 * (steps of the lane's current game), sel uint8[n] (the lane is active: the lane selection
 * of bgx_one_ply_sel / bgx_two_ply_sel), tally int64[n_groups][8] (bgx_rollout_field) and
 * active int64[1].  A win is a win by the start record's mover (byte 52 of
 * starts_dev[i]); 1 / 2 / 3 is info's game_score.  records_dev = the engine's lane records.
 * No entry point synchronises or allocates: both can be captured into a HIP graph.
 * bgx_rollout_begin: zeroes the state, sel from group and games_per_lane, active = the
 * number of active lanes.
 * bgx_rollout_advance: after bgx_step, with that step's done and info.  Every active lane
 * adds a ply to its own counter; a done with a winner adds the game, its plies and its
 * result to the lane's group row and zeroes the counter; a lane that finished its last game
 * is deselected and active drops.  The sums are integers: run-to-run identical.
 * BGX_EINVAL for n <= 0, n_groups <= 0, games_per_lane < 0 or a NULL pointer. */
enum bgx_rollout_field {
    BGX_ROLLOUT_GAMES = 0,        /* finished games */
    BGX_ROLLOUT_PLIES = 1,        /* their steps, passes included */
    BGX_ROLLOUT_WIN1 = 2,  BGX_ROLLOUT_WIN2 = 3,  BGX_ROLLOUT_WIN3 = 4,    /* won by the start mover: 1 / 2 / 3 points */
    BGX_ROLLOUT_LOSS1 = 5, BGX_ROLLOUT_LOSS2 = 6, BGX_ROLLOUT_LOSS3 = 7
};
int bgx_rollout_begin(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* group_dev, int32_t n,
                      int32_t n_groups, int32_t games_per_lane, int32_t* games_done_dev, int32_t* plies_dev,
                      uint8_t* sel_dev, int64_t* tally_dev, int64_t* active_dev, void* stream);
int bgx_rollout_advance(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* group_dev,
                        const uint8_t* done_dev, const int32_t* info_dev, int32_t n, int32_t n_groups,
                        int32_t games_per_lane, int32_t* games_done_dev, int32_t* plies_dev, uint8_t* sel_dev,
                        int64_t* tally_dev, int64_t* active_dev, void* stream);

/* Luck bookkeeping of a rollout (DESIGN.md §10 "Luck adjustment"), beside the state above:
 * lane_luck float[n] (the running sum of the lane's current game) and luck_tally
 * int64[n_groups][4] (bgx_rollout_luck_field), both zeroed by the caller.  A game's luck L is
 * the fp32 sum, in step order, of s * luck over its steps, s = +1 when the step's mover is
 * the start record's mover, else -1.  Plain kernels, no allocation and no synchronisation:
 * graph-capturable.
 * bgx_rollout_luck_add: before the players act, with luck_dev = bgx_roll_luck's luck_out for
 * the lanes as they stand.  Every lane with sel[i] != 0, except in the first step of a game
 * (plies[i] == 0) whose start record fixed the roll (byte 53 of starts_dev[i] non-zero: that
 * roll was not drawn, so it has no luck): lane_luck[i] += records[i][52] == starts[i][52] ?
 * luck[i] : -luck[i] (one fp32 add).
 * bgx_rollout_luck_flush: after bgx_step and BEFORE bgx_rollout_advance (sel is still the
 * step's selection), with the step's done and info.  A lane with sel[i] != 0, a valid group
 * and a game that bgx_rollout_advance counts (done with a winner) adds, with
 * Lq = llrintf(lane_luck[i] * 65536) clamped to +-2^21 (0 when not finite; round half even)
 * and res = +-game_score from the start mover's side, to row group[i]:
 *   LUCK += Lq, LUCK2 += Lq * Lq, RESLUCK += res * Lq, LUCK_GAMES += 1,
 * and lane_luck[i] = 0; any other done of a selected lane only zeroes lane_luck[i].  The sums
 * are integers: run-to-run identical.  Range: Lq^2 <= 2^42, so a row holds 2^21 games at the
 * clamp (|L| = 32 points each) before LUCK2 could pass 2^63.
 * BGX_EINVAL for n <= 0, n_groups <= 0 or a NULL pointer. */
enum bgx_rollout_luck_field {
    BGX_ROLLOUT_LUCK = 0,         /* sum of Lq (2^-16 points) */
    BGX_ROLLOUT_LUCK2 = 1,        /* sum of Lq^2 (2^-32) */
    BGX_ROLLOUT_RESLUCK = 2,      /* sum of res * Lq (2^-16) */
    BGX_ROLLOUT_LUCK_GAMES = 3    /* games added: equals BGX_ROLLOUT_GAMES of the row */
};
int bgx_rollout_luck_add(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* plies_dev,
                         const uint8_t* sel_dev, const float* luck_dev, int32_t n, float* lane_luck_dev, void* stream);
int bgx_rollout_luck_flush(const uint8_t* starts_dev, const int32_t* group_dev, const uint8_t* sel_dev,
                           const uint8_t* done_dev, const int32_t* info_dev, int32_t n, int32_t n_groups,
                           float* lane_luck_dev, int64_t* luck_tally_dev, void* stream);

/* ---- exact two-sided bearoff database (csrc/bg_bearoff.h; bgx/bearoff.py; no
 * counterpart in the reference) ----
 * Once both sides have at most K checkers left, all on their own home points, the cubeless game
 * is a race between two independent six-point configurations and its value under perfect play
 * is a finite dynamic program.  A configuration is the six counts c[d-1], d = 1..6 = checkers
 * at distance d from bearing off (PLAYER1: point 24 - d, PLAYER2: point d - 1), sum <= K;
 * there are n = C(K + 6, 6) of them, ordered by (pip count sum_d d c[d-1], then the base-9
 * number sum_d c[d-1] 9^(d-1)) ascending: index 0 is the empty one and every pip count is a
 * contiguous range.  bgx_bearoff_buffers publishes the order, so no caller needs the formula:
 *   configs  int8[n][6]      the counts of configuration i
 *   succ_off int32[n*21+1], succ int32[]   for configuration a and roll r (bgx_two_ply's roll
 *            order), succ[succ_off[21 a + r] .. succ_off[21 a + r + 1]) = the distinct
 *            configurations a legal play of r reaches, ascending (both dice when possible, the
 *            reference's move generator restricted to a bearoff board: the opponent neither
 *            blocks nor is hit); a roll that cannot be played gives a itself
 *   table    float[n][n]     W[a][b] = the probability that the side ON ROLL with a wins
 *            against b when both sides maximise their win probability:
 *              W[a][empty] = 0,  W[empty][b] = 1 (b not empty),  otherwise
 *              w_r = max over a' in succ(a, r) of (a' empty ? 1 : 1 - W[b][a'])
 *              W[a][b] = sum over r = 0..20, in that order from 0.0f, of p_r * w_r,
 *            p_r = fp32(1/36) for doubles and fp32(2/36) otherwise, every subtraction, product
 *            and sum rounded to fp32 once (no fma): the value does not depend on the schedule
 *            or on K, and a numpy float32 loop reproduces it bit for bit.
 * Equity in points is 2 W - 1: with K <= 8 both sides have checkers off, so a game is single.
 * bgx_bearoff_create: 1 <= max_checkers <= 8 (else BGX_EINVAL); allocates and builds on
 * `stream` (successor sets: count, scan, fill; then one launch per total pip count) and
 * synchronises it (it sizes succ from the count pass); BGX_EOVERFLOW if a successor set
 * outgrew its room (none does for K <= 8).  bgx_bearoff_destroy synchronises the device. */
typedef struct bgx_bearoff bgx_bearoff;
typedef struct {
    const float* table;
    const int8_t* configs;
    const int32_t* succ_off;   /* [n*21+1] */
    const int32_t* succ;
    int32_t n, max_checkers;
} bgx_bearoff_buffers;
int bgx_bearoff_create(int device, int32_t max_checkers, void* stream, bgx_bearoff** out);
int bgx_bearoff_buffers_get(bgx_bearoff* db, bgx_bearoff_buffers* out);
int bgx_bearoff_destroy(bgx_bearoff* db);

/* One thread per 64-byte lane record (records_dev 16-byte aligned), on the caller's stream as
 * given, like bgx_policy_act.  A record is in the table when game_over (byte 55) is 0, both
 * bars are empty, each side has between 1 and K checkers on the board, all of them on its own
 * six home points, and points + off == 15 for both sides.  Then in_db_out[i] = 1 and
 * win_out[i] = W[cfg(mover)][cfg(opponent)], the mover's exact win probability before its
 * roll (the roll bytes are not read); else in_db_out[i] = 0 and win_out[i] is not written.
 * win_out may be NULL.  No allocation, no synchronisation: graph-capturable. */
int bgx_bearoff_lookup(const bgx_bearoff* db, const uint8_t* records_dev, int32_t n, uint8_t* in_db_out,
                       float* win_out, void* stream);

/* Perfect play on the engine's lanes; ordered like every engine call.  For each lane with
 * lane_sel_dev[i] != 0 (NULL = every lane) whose record is in the table and which has a legal
 * move: every move of the engine's list (bgx_buffers.moves, count in bytes 60-61) gives the
 * mover's afterstate configuration a' from its sub-moves (start point minus one, end point
 * plus one unless BEAR_OFF), and act_inout[i] = the first argmax of
 * (a' empty ? 1 : 1 - W[cfg(opponent)][a']).  Other lanes' entries are not written.
 * in_db_out (uint8[B], may be NULL) receives the table test of the selected lanes and 0 for
 * the others.  No allocation, no synchronisation: graph-capturable.  BGX_EINVAL when the
 * database lives on another device than the engine. */
int bgx_bearoff_act(bgx_engine* e, const bgx_bearoff* db, const uint8_t* lane_sel_dev, int32_t* act_inout,
                    uint8_t* in_db_out, void* stream);

/* Rollout cut: a game that reaches the table is stopped and scored with its exact win
 * probability.  Beside the state of bgx_rollout_begin / bgx_rollout_advance: cut_tally
 * int64[n_groups][4] (bgx_rollout_cut_field), zeroed by the caller, and reset_mask_out
 * uint8[n].  Call it once after bgx_rollout_begin and after every bgx_rollout_advance.  A lane
 * with sel[i] != 0, a valid group and a record in the table (bgx_bearoff_lookup's test):
 *   q = W when the record's mover (byte 52) is the start record's mover, else 1 - W (fp32);
 *   Pq = llrintf(q * 1048576.0f) clamped to [0, 2^20];
 *   row group[i]: CUT_GAMES += 1, CUT_PLIES += plies[i], CUT_P += Pq, CUT_P2 += Pq * Pq;
 *   games_done[i] += 1, plies[i] = 0; the lane's last game: sel[i] = 0 and active drops;
 *   reset_mask_out[i] = 1.
 * Every other lane gets reset_mask_out[i] = 0.  The caller then runs bgx_reset with that mask,
 * which gives each cut lane its start record again.  The sums are integers: run-to-run
 * identical; Pq^2 <= 2^40, so a row holds 2^23 cut games.  No allocation, no synchronisation:
 * graph-capturable.  BGX_EINVAL for n <= 0, n_groups <= 0, games_per_lane < 0, a NULL pointer
 * or records that are not 16-byte aligned. */
enum bgx_rollout_cut_field {
    BGX_ROLLOUT_CUT_GAMES = 0,    /* cut games */
    BGX_ROLLOUT_CUT_PLIES = 1,    /* their steps */
    BGX_ROLLOUT_CUT_P = 2,        /* sum of Pq (2^-20) */
    BGX_ROLLOUT_CUT_P2 = 3        /* sum of Pq^2 (2^-40) */
};
int bgx_rollout_bearoff_cut(const bgx_bearoff* db, const uint8_t* records_dev, const uint8_t* starts_dev,
                            const int32_t* group_dev, int32_t n, int32_t n_groups, int32_t games_per_lane,
                            int32_t* games_done_dev, int32_t* plies_dev, uint8_t* sel_dev, int64_t* cut_tally_dev,
                            int64_t* active_dev, uint8_t* reset_mask_out, void* stream);

/* ---- one-sided bearoff database (csrc/bg_bearoff1.h; bgx/bearoff.py; no
 * counterpart in the reference) ----
 * For every configuration of ONE side's home board with at most K checkers, 1 <= K <= 15, the
 * distribution of the number of rolls the side needs to bear everything off when it plays to
 * minimise the mean of that number.  Two rows give the win probability of any race between two
 * home boards -- an approximation (each side plays its own race and ignores the other's), where
 * the two-sided table above is exact; DESIGN.md §12 has the measured distance.
 * Configurations are those of the two-sided table (six counts c[d-1], sum <= K), n = C(K + 6, 6)
 * of them (54,264 at K = 15), ordered by (pip count, then the base-16 number
 * sum_d c[d-1] 16^(d-1)) ascending: index 0 is the empty one, every pip count is a contiguous
 * range, and for K <= 8 the order is the two-sided table's (both are lexicographic on
 * (c6, ..., c1) within a pip count).  succ(a, r) is the two-sided table's successor set, for
 * the 21 rolls in bgx_two_ply's order.  With T = 32 entries a row and every product,
 * difference and sum rounded to fp32 once (no fma):
 *   D[empty][0] = 1, D[empty][t > 0] = 0;  mean[empty] = 0
 *   choice[a][r] = the a' in succ(a, r) with the smallest (mean[a'], index a'), lexicographic
 *                  (fp32 means tie, so the index decides); choice[empty][r] = empty
 *   D[a][0] = 0;  D[a][t] = sum over r = 0..20, in that order from 0.0f, of
 *                  p_r * D[choice[a][r]][t - 1],  t = 1..31
 *   mean[a] = sum over t = 1..31, in that order from 0.0f, of fp32(t) * D[a][t]
 *   S[a][0] = S[a][1] = 1.0f;  S[a][t + 1] = S[a][t] - D[a][t]      (a not empty;
 *                  S[a][t] = P(a needs >= t rolls));  S[empty] = (1, 0, 0, ...)
 *   win1(x on roll, y) = sum over t = 1..31, in that order from 0.0f, of D[x][t] * S[y][t]
 *                  (x, y not empty): x wins when it needs no more rolls than y
 * with p_r as above.  A numpy float32 loop reproduces every entry bit for bit.  At K = 15 the
 * last non-zero entry of a row is at t = 30.  bgx_bearoff1_buffers:
 *   dist float[n][32] = D,  surv float[n][32] = S,  mean float[n],  choice int32[n][21],
 *   configs int8[n][6] the counts of configuration i.
 * bgx_bearoff1_create: 1 <= max_checkers <= 15 (else BGX_EINVAL); allocates and builds on
 * `stream`, two launches per pip count, and synchronises it once at the end; BGX_EOVERFLOW when
 * a row has a non-zero D[a][31] (none does).  bgx_bearoff1_destroy synchronises the device. */
typedef struct bgx_bearoff1 bgx_bearoff1;
typedef struct {
    const float* dist;
    const float* surv;
    const float* mean;
    const int32_t* choice;
    const int8_t* configs;
    int32_t n, max_checkers;
} bgx_bearoff1_buffers;
int bgx_bearoff1_create(int device, int32_t max_checkers, void* stream, bgx_bearoff1** out);
int bgx_bearoff1_buffers_get(bgx_bearoff1* db, bgx_bearoff1_buffers* out);
int bgx_bearoff1_destroy(bgx_bearoff1* db);

/* bgx_bearoff_lookup's record test with this table's K (a side may have all 15 checkers on the
 * board).  in_db_out[i] = 1: in the table and both sides have borne a checker off, so every game
 * from here is a single one and the equity is 2 win - 1; 2: in the table with all 15 checkers of
 * a side on the board: win_out is still the win probability, but gammons are possible and it is
 * no equity; 0: not in the table, win_out[i] is not written.  Where in_db_out[i] != 0,
 * win_out[i] = win1(cfg(mover), cfg(opponent)).  win_out may be NULL.  No allocation, no
 * synchronisation: graph-capturable. */
int bgx_bearoff1_lookup(const bgx_bearoff1* db, const uint8_t* records_dev, int32_t n, uint8_t* in_db_out,
                        float* win_out, void* stream);

/* bgx_bearoff_act's contract on this table: for each selected lane whose record is in the table
 * (in_db 1 or 2) and which has a legal move, act_inout[i] = the first argmax over the engine's
 * move list of (a' empty ? 1 : 1 - win1(cfg(opponent), a')): it plays for the win given both
 * sides' rows, which is better than minimising its own mean.  in_db_out receives the test's
 * value (0, 1, 2) of the selected lanes and 0 for the others. */
int bgx_bearoff1_act(bgx_engine* e, const bgx_bearoff1* db, const uint8_t* lane_sel_dev, int32_t* act_inout,
                     uint8_t* in_db_out, void* stream);

/* bgx_rollout_bearoff_cut with W = win1(cfg(mover), cfg(opponent)): the same arguments, sums,
 * fixed point and reset mask.  It cuts only the lanes whose test gives 1: with 15 checkers of a
 * side on the board the game may still be a gammon and is played on. */
int bgx_rollout_bearoff1_cut(const bgx_bearoff1* db, const uint8_t* records_dev, const uint8_t* starts_dev,
                             const int32_t* group_dev, int32_t n, int32_t n_groups, int32_t games_per_lane,
                             int32_t* games_done_dev, int32_t* plies_dev, uint8_t* sel_dev, int64_t* cut_tally_dev,
                             int64_t* active_dev, uint8_t* reset_mask_out, void* stream);

/* ---- the doubling cube in position rollouts, money play (csrc/bg_cube.h; bgx/cube.py,
 * bgx/rollout.py; no counterpart in the reference) ----
 * Beside the state of bgx_rollout_begin / bgx_rollout_advance: cube uint8[n], the cube of the
 * lane's current game, and cube0 uint8[n], the cube each game on lane i starts with, both the
 * caller's device arrays.  A state byte: bits 0-3 = k (the cube shows 2^k, 0 <= k <= 10), bits
 * 4-5 = the owner (0 centred, 1 PLAYER1 = mover byte 0, 2 PLAYER2).  A byte is valid when
 * k <= cap, owner <= 2 and owner == 0 exactly when k == 0; the kernels read k as min(k, cap) and
 * owner 3 as 0, so they are defined on any byte.  cube_tally int64[n_groups][8]
 * (bgx_rollout_cube_field) is zeroed by the caller.  The rule is passed by value:
 *   scale, double_at, pass_at, too_good_at: with e = scale * equity in fp32 (one product), the
 *     side on roll doubles iff double_at <= e <= too_good_at (a NaN never doubles), and the
 *     opponent passes iff e > pass_at, else it takes;
 *   cap: no double at k == cap (0..10);  jacoby != 0: a game that ends with the cube at k == 0
 *     counts 1 point, gammon or not.
 * Per step: cube_sel, the equity of the dsel lanes (bgx_roll_luck's mean_out with dsel as its
 * lane selection, or any other source), cube_decide, bgx_reset with the mask, the players' act,
 * bgx_step, cube_flush, bgx_rollout_advance; cube_begin once after bgx_rollout_begin.
 * bgx_rollout_cube_begin: cube[i] = cube0[i], sanitised as above.
 * bgx_rollout_cube_sel: dsel_out[i] = 1 when sel[i] != 0, the group is valid, plies[i] > 0 (no
 * cube action on a game's first ply), the record is not game_over (byte 55), k < cap and the cube
 * is centred or owned by the record's mover; else 0.
 * bgx_rollout_cube_decide: for a lane with dsel[i] != 0 and a valid group, m = the record's mover
 * and equity[i] = m's own equity before its roll (cube_sel's test of the cube itself, k < cap and
 * centred or m's own, is made again, so a dsel of another origin cannot take the cube past the
 * cap).  The mover doubles and the opponent
 * passes: the game ends worth y = +-(1 << k), positive when m is the start record's mover (byte
 * 52 of starts_dev[i]); row group[i]: CUBE_GAMES += 1, CUBE_POINTS += y, CUBE_POINTS2 += y * y,
 * CUBE_LOG2 += k, PASS_GAMES += 1, PASS_PLIES += plies[i], PASS_WON += (y > 0), DOUBLES += 1;
 * games_done[i] += 1, plies[i] = 0; the lane's last game: sel[i] = 0 and active drops;
 * cube[i] = cube0[i]; reset_mask_out[i] = 1.  The mover doubles and the opponent takes: k += 1,
 * owner = 2 - m (the other side), DOUBLES += 1.  Every other lane gets reset_mask_out[i] = 0 and
 * is otherwise untouched.  The caller then runs bgx_reset with the mask.
 * bgx_rollout_cube_flush: after bgx_step and BEFORE bgx_rollout_advance, with the step's done and
 * info.  A lane with sel[i] != 0, a valid group and a game that bgx_rollout_advance counts (done
 * with a winner): s = info's game_score, or 1 when rule.jacoby and k == 0; y = +-(s << k) from
 * the start mover's side; CUBE_GAMES += 1, CUBE_POINTS += y, CUBE_POINTS2 += y * y,
 * CUBE_LOG2 += k; then cube[i] = cube0[i].  Any other done of a selected lane only resets the
 * cube.  |y| <= 3 * 2^10, so y^2 < 2^24 and a row holds 2^39 games.  The sums are integers:
 * run-to-run identical, and CUBE_GAMES = BGX_ROLLOUT_GAMES of the plain tally + PASS_GAMES.
 * Plain kernels, one thread per lane, no allocation and no synchronisation: graph-capturable.
 * BGX_EINVAL for n <= 0, n_groups <= 0, games_per_lane < 0, a NULL pointer, cap outside 0..10 or
 * a NaN in scale, double_at or pass_at (too_good_at may be +inf). */
typedef struct {
    float scale, double_at, pass_at, too_good_at;
    int32_t cap;
    int32_t jacoby;
} bgx_cube_rule;
enum bgx_rollout_cube_field {
    BGX_ROLLOUT_CUBE_GAMES = 0,       /* games that ended, played out or passed */
    BGX_ROLLOUT_CUBE_POINTS = 1,      /* sum of y, points from the start mover's side */
    BGX_ROLLOUT_CUBE_POINTS2 = 2,     /* sum of y^2 */
    BGX_ROLLOUT_CUBE_LOG2 = 3,        /* sum of k at the game's end */
    BGX_ROLLOUT_CUBE_PASS_GAMES = 4,  /* games ended by a passed double */
    BGX_ROLLOUT_CUBE_PASS_PLIES = 5,  /* their steps */
    BGX_ROLLOUT_CUBE_PASS_WON = 6,    /* of them, won by the start mover */
    BGX_ROLLOUT_CUBE_DOUBLES = 7      /* doubles offered, taken or passed */
};
int bgx_rollout_cube_begin(const uint8_t* cube0_dev, int32_t n, int32_t cap, uint8_t* cube_dev, void* stream);
int bgx_rollout_cube_sel(const uint8_t* records_dev, const int32_t* group_dev, int32_t n_groups,
                         const int32_t* plies_dev, const uint8_t* sel_dev, const uint8_t* cube_dev, int32_t n,
                         int32_t cap, uint8_t* dsel_out, void* stream);
int bgx_rollout_cube_decide(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* group_dev,
                            const uint8_t* dsel_dev, const float* equity_dev, int32_t n, int32_t n_groups,
                            int32_t games_per_lane, bgx_cube_rule rule, const uint8_t* cube0_dev, uint8_t* cube_dev,
                            int32_t* games_done_dev, int32_t* plies_dev, uint8_t* sel_dev, int64_t* cube_tally_dev,
                            int64_t* active_dev, uint8_t* reset_mask_out, void* stream);
int bgx_rollout_cube_flush(const uint8_t* starts_dev, const int32_t* group_dev, const uint8_t* sel_dev,
                           const uint8_t* done_dev, const int32_t* info_dev, int32_t n, int32_t n_groups,
                           bgx_cube_rule rule, const uint8_t* cube0_dev, uint8_t* cube_dev, int64_t* cube_tally_dev,
                           void* stream);

/* ---- the doubling cube in the head-to-head arena, money play (csrc/bg_arena_cube.h;
 * bgx/arena.py; no counterpart in the reference) ----
 * The rule of the block above in two halves, each taken by a different party: the side on roll
 * offers a double by its own rule on its own equity, the other side answers by its own rule on
 * its own estimate of the doubler's equity.  Beside the state of bgx_arena_begin (games_done,
 * sel_a, sel_b, tally) the caller owns cube uint8[n], the state byte of the lane's current game
 * (as above; every arena game starts centred at 1, byte 0), plies int32[n], the steps of the
 * lane's current game, and cube_tally int64[16] (bgx_arena_cube_field).  rule_a / rule_b are A's
 * and B's bgx_cube_rule; cap and jacoby belong to the game, so the two must agree on them.  Seat
 * rule as in the arena: in game g of lane i, A is PLAYER1 iff ((i + g) & 1) == 0.
 * Per step: cube_sel; A's equity on dsel_a and B's on dsel_b; cube_offer; B's equity on off_a and
 * A's on off_b (the doubler's equity, the mover's view, as the responder estimates it);
 * cube_respond; bgx_reset with the mask; cube_reseat; the players' act; bgx_arena_merge; bgx_step;
 * cube_flush; bgx_arena_advance.  cube_begin once after bgx_arena_begin.
 * bgx_arena_cube_begin: cube = 0, plies = 0, cube_tally = 0.
 * bgx_arena_cube_sel: dsel_x_out[i] = 1 when sel_x[i] != 0, plies[i] > 0 (no cube action on a
 * game's first ply), the record is not game_over (byte 55), k < cap and the cube is centred or
 * owned by the record's mover; else 0 (x = a, b).
 * bgx_arena_cube_offer: off_a_out[i] = 1 when dsel_a[i] != 0, the cube is open to the record's
 * mover (cube_sel's test of the cube itself, made again: a dsel of another origin cannot take
 * the cube past the cap) and, with e = rule_a.scale * eq_a[i] in fp32 (one product),
 * rule_a.double_at <= e <= rule_a.too_good_at (a NaN never doubles); else 0.  off_b_out likewise
 * from dsel_b, eq_b and rule_b.  DOUBLES_A += the off_a lanes, DOUBLES_B += the off_b lanes.
 * bgx_arena_cube_respond: on a lane with off_a[i] != 0 B answers: it passes iff rule_b.scale *
 * eq_b[i] > rule_b.pass_at (a NaN takes); on a lane with off_b[i] != 0 (and off_a[i] == 0) A
 * answers by rule_a on eq_a[i].  Only active lanes (games_done[i] < games_per_lane) whose cube is
 * open to the record's mover m are answered.  Take: k += 1, owner = 2 - m (the taker).  Pass: the
 * game ends worth y = +(1 << k) to A when A doubled, -(1 << k) when B did; CUBE_GAMES += 1,
 * CUBE_POINTS_A += y, CUBE_POINTS2 += y * y, CUBE_WINS_A += (y > 0), CUBE_LOG2 += k,
 * PASS_GAMES += 1, PASS_PLIES += plies[i], PASSES_A += 1 when A gave up, else PASSES_B += 1;
 * games_done[i] += 1, plies[i] = 0, cube[i] = 0, sel_a[i] = sel_b[i] = 0 (until the reseat); the
 * lane's last game: tally[BGX_ARENA_ACTIVE] drops; reset_mask_out[i] = 1.  Every other lane gets
 * reset_mask_out[i] = 0.  The caller then runs bgx_reset with the mask.
 * bgx_arena_cube_reseat: after that reset.  A lane with reset_mask[i] != 0 and games_done[i] <
 * games_per_lane gets sel_a / sel_b from the new record's mover and the new g = games_done[i].
 * bgx_arena_cube_flush: after bgx_step and BEFORE bgx_arena_advance, with the step's done and
 * info, while games_done[i] is still the finished game's g.  For a lane with sel_a[i] or sel_b[i]
 * set (an active lane): a done with a winner is scored at the cube, s = info's game_score, or 1
 * when jacoby != 0 and k == 0, y = +-(s << k) from A's side: CUBE_GAMES += 1, CUBE_POINTS_A += y,
 * CUBE_POINTS2 += y * y, CUBE_WINS_A += (y > 0), CUBE_LOG2 += k; then cube[i] = 0, plies[i] = 0.
 * Any other done only resets cube and plies; a lane without a done gets plies[i] += 1.
 * The plain tally keeps counting the games played to the end only, as a rollout's does (its
 * PLIES counts every step of an active lane).  CUBE_GAMES == tally[BGX_ARENA_GAMES] + PASS_GAMES
 * and PASS_GAMES == PASSES_A + PASSES_B; |y| <= 3 * 2^10; all sums are integers, hence
 * run-to-run identical.  Plain kernels, one thread per lane, no allocation and no
 * synchronisation: graph-capturable.  BGX_EINVAL for n <= 0, games_per_lane < 0, a NULL pointer,
 * cap outside 0..10, a NaN in a rule's scale, double_at or pass_at (too_good_at may be +inf), or
 * rules that differ in cap or jacoby. */
enum bgx_arena_cube_field {
    BGX_ARENA_CUBE_GAMES = 0,        /* games that ended, played out or passed */
    BGX_ARENA_CUBE_POINTS_A = 1,     /* sum of y, points from A's side */
    BGX_ARENA_CUBE_POINTS2 = 2,      /* sum of y^2 */
    BGX_ARENA_CUBE_WINS_A = 3,       /* games with y > 0 */
    BGX_ARENA_CUBE_LOG2 = 4,         /* sum of k at the game's end */
    BGX_ARENA_CUBE_PASS_GAMES = 5,   /* games ended by a passed double */
    BGX_ARENA_CUBE_PASS_PLIES = 6,   /* their steps */
    BGX_ARENA_CUBE_PASSES_A = 7,     BGX_ARENA_CUBE_PASSES_B = 8,   /* the side that gave up */
    BGX_ARENA_CUBE_DOUBLES_A = 9,    BGX_ARENA_CUBE_DOUBLES_B = 10  /* doubles offered; 11..15 stay zero */
};
int bgx_arena_cube_begin(int32_t n, uint8_t* cube_dev, int32_t* plies_dev, int64_t* cube_tally_dev, void* stream);
int bgx_arena_cube_sel(const uint8_t* records_dev, const uint8_t* sel_a_dev, const uint8_t* sel_b_dev,
                       const int32_t* plies_dev, const uint8_t* cube_dev, int32_t n, int32_t cap, uint8_t* dsel_a_out,
                       uint8_t* dsel_b_out, void* stream);
int bgx_arena_cube_offer(const uint8_t* records_dev, const uint8_t* dsel_a_dev, const uint8_t* dsel_b_dev,
                         const float* eq_a_dev, const float* eq_b_dev, bgx_cube_rule rule_a, bgx_cube_rule rule_b,
                         const uint8_t* cube_dev, int32_t n, uint8_t* off_a_out, uint8_t* off_b_out,
                         int64_t* cube_tally_dev, void* stream);
int bgx_arena_cube_respond(const uint8_t* records_dev, const uint8_t* off_a_dev, const uint8_t* off_b_dev,
                           const float* eq_a_dev, const float* eq_b_dev, bgx_cube_rule rule_a, bgx_cube_rule rule_b,
                           int32_t n, int32_t games_per_lane, uint8_t* cube_dev, int32_t* plies_dev,
                           int32_t* games_done_dev, uint8_t* sel_a_dev, uint8_t* sel_b_dev, int64_t* tally_dev,
                           int64_t* cube_tally_dev, uint8_t* reset_mask_out, void* stream);
int bgx_arena_cube_reseat(const uint8_t* records_dev, const uint8_t* reset_mask_dev, int32_t n, int32_t games_per_lane,
                          const int32_t* games_done_dev, uint8_t* sel_a_dev, uint8_t* sel_b_dev, void* stream);
int bgx_arena_cube_flush(const uint8_t* sel_a_dev, const uint8_t* sel_b_dev, const uint8_t* done_dev,
                         const int32_t* info_dev, const int32_t* games_done_dev, int32_t n, int32_t jacoby, int32_t cap,
                         uint8_t* cube_dev, int32_t* plies_dev, int64_t* cube_tally_dev, void* stream);

/* ---- match play in the arena: matches to L points, Crawford rule, cube decisions on a match
 * equity table (csrc/bg_match.h; bgx/match.py, bgx/arena.py; no counterpart in the
 * reference) ----
 * Beside the state of bgx_arena_begin the caller owns, per lane: away uint8[n, 2], the points A
 * and B still need, each in 1..L (L = length in 1..25); craw uint8[n], 0 before the Crawford game,
 * 1 the Crawford game, 2 after it; cube uint8[n], the cube byte of the blocks above, read with cap
 * 10; plies int32[n]; matches_done int32[n]; seat0 uint8[n], 1 when A sat as PLAYER1 in the first
 * game of the lane's current match; retire uint8[n], flush's note to retire; and match_tally
 * int64[16] (bgx_arena_match_field).
 * The tables: met float[(L + 1)^2], met[i (L + 1) + j] the chance that the side needing i wins the
 * match against the side needing j at the start of a game; rows and columns at 1 hold the Crawford
 * game's values.  pc float[L + 1]: pc[j] the trailer's chance after the Crawford game when it
 * needs j and the leader 1; pc[1] = 0.5.  met_after(me, opp, craw_now) is the value of the next
 * game after this game's points are taken off: me <= 0 gives 1, opp <= 0 gives 0; with craw_now !=
 * 0 the next game is post-Crawford: me == 1 gives 1 - pc[opp], else pc[me]; with craw_now == 0 it
 * is met[me][opp].  Indices past L read L: the function is total.
 * The rule of a side, bgx_match_rule: window in [0, 1]; win_gammons / loss_gammons in [0, 1], the
 * share of the owner's wins / losses that are gammons (backgammons are not modelled).  Every fp32
 * product, sum and difference below is rounded once, none contracted.
 * Win probability of the side on roll from a value v: gw = the owner's win_gammons, gl = its
 * loss_gammons when the owner is on roll, swapped when the owner answers a double (it then
 * evaluates the doubler's chances); W = 1 + gw, L_ = 1 + gl; c = scale v clamped to [-L_, W] by
 * comparisons (a NaN stays a NaN); p = (c + L_) / (W + L_).
 * The side on roll needs x, the other y, the cube shows v = 2^k:
 *   win(n)  = (1 - gw) met_after(x - n, y) + gw met_after(x - 2n, y)
 *   loss(n) = (1 - gl) (1 - met_after(y - n, x)) + gl (1 - met_after(y - 2n, x))
 *   ND = loss(v) + p (win(v) - loss(v));  DT = loss(2v) + p (win(2v) - loss(2v));  DP = met_after(x - v, y)
 * Access, the side on roll may double: plies > 0, the record not game_over, the lane active, craw
 * != 1, the cube below 2^10 and centred or the mover's, and x > v (else the cube is dead for a side
 * that wins the match with this game anyway).
 * Offer: with access the side on roll doubles iff ND <= DP (not too good) and either DT - ND >=
 * window (DP - ND) (window 0 the dead-cube doubling point, 1 the cash point) or y <= v and DT > ND
 * (the free double: losing this game loses the match at any cube).  A NaN never doubles.
 * Answer: the other side passes iff DT' > DP' in its own numbers: its own value of the position
 * (the doubler's value as it estimates it), its own scale, its shares swapped.  A tie or a NaN
 * takes.  Take: k += 1, owner = 2 - m (the taker).  Pass: the doubler scores v points.
 * End of a game: the winner's away drops by s 2^k, s = info's game_score for a played-out game (no
 * Jacoby rule in a match), 1 for a pass.  Winner's away <= 0: the match ends, away = (L, L), craw =
 * 0, matches_done += 1.  Else craw 0 -> 1 when the winner's away is now 1, and 1 -> 2.  cube = 0,
 * plies = 0.
 * The quota is matches: bgx_arena_begin / bgx_arena_advance / bgx_arena_cube_reseat are called
 * with games_per_lane = matches_per_lane (2 L - 1) (it must fit int32), which no lane reaches by
 * playing, and a lane that finishes its last match is retired by games_done = games_per_lane,
 * sel_a = sel_b = 0 and tally[BGX_ARENA_ACTIVE] -= 1: by match_respond on a pass, by match_retire
 * after bgx_arena_advance has counted the game on a played-out one.  The plain tally counts the
 * played-out games of counted matches.
 * Per step: match_sel; A's value on dsel_a and B's on dsel_b; match_offer; B's value on off_a and
 * A's on off_b; match_respond; bgx_reset with the mask; bgx_arena_cube_reseat; the players' act;
 * bgx_arena_merge; bgx_step; match_flush; bgx_arena_advance; match_retire.  match_begin once after
 * bgx_arena_begin.
 * bgx_arena_match_begin: away = (L, L), craw = cube = plies = matches_done = retire = 0, seat0 =
 * the seat of game 0, match_tally = 0.
 * bgx_arena_match_sel: dsel_x_out[i] = 1 when sel_x[i] != 0 and side x has access; else 0.
 * bgx_arena_match_offer: off_x_out[i] = 1 when sel_x[i] != 0, dsel_x[i] != 0, access holds (tested
 * again) and side x offers by rule_x on eq_x[i]; DOUBLES_A / DOUBLES_B count them.
 * bgx_arena_match_respond: on an active lane with access, sel_a and off_a set, B answers by rule_b
 * on eq_b[i]; with sel_b and off_b set, A by rule_a on eq_a[i].  A pass scores the game (GAMES,
 * PASS_GAMES, POINTS_x, PASSES_x of the side that gave up, LOG2 += k, PASS_PLIES += plies, the
 * Crawford counts and the match counts), games_done += 1 (or = games_per_lane: the lane's last
 * match), sel_a = sel_b = 0 until the reseat, reset_mask_out[i] = 1; every other lane gets 0.
 * bgx_arena_match_flush: after bgx_step and BEFORE bgx_arena_advance.  On a lane with sel_a or
 * sel_b set: a done with a winner is scored at the cube's value as above; the lane's last match
 * sets retire[i] = 1.  Any done resets cube and plies; a lane without a done gets plies += 1.
 * bgx_arena_match_retire: after bgx_arena_advance: retires the flagged lanes, clears the flag.
 * All sums are integers, hence run-to-run identical.  Plain kernels, one thread per lane, no
 * allocation and no synchronisation: graph-capturable.  BGX_EINVAL for n <= 0, a NULL pointer,
 * length outside 1..25, matches_per_lane < 0, games_per_lane != matches_per_lane (2 length - 1)
 * (match_respond), a NaN scale, or window or a gammon share outside [0, 1] (a NaN included). */
typedef struct {
    float scale, window, win_gammons, loss_gammons;
} bgx_match_rule;
enum bgx_arena_match_field {
    BGX_ARENA_MATCH_MATCHES = 0,              /* matches that ended */
    BGX_ARENA_MATCH_WINS_A = 1,               /* of them, won by A */
    BGX_ARENA_MATCH_GAMES = 2,                /* games that ended, played out or passed */
    BGX_ARENA_MATCH_PASS_GAMES = 3,           /* games ended by a passed double */
    BGX_ARENA_MATCH_POINTS_A = 4,             BGX_ARENA_MATCH_POINTS_B = 5,   /* cube-multiplied points scored */
    BGX_ARENA_MATCH_DOUBLES_A = 6,            BGX_ARENA_MATCH_DOUBLES_B = 7,  /* doubles offered */
    BGX_ARENA_MATCH_PASSES_A = 8,             BGX_ARENA_MATCH_PASSES_B = 9,   /* the side that gave up */
    BGX_ARENA_MATCH_LOG2 = 10,                /* sum of k at the game's end */
    BGX_ARENA_MATCH_CRAWFORD_GAMES = 11,      /* games played as the Crawford game */
    BGX_ARENA_MATCH_POST_CRAWFORD_GAMES = 12, /* games played after it */
    BGX_ARENA_MATCH_PASS_PLIES = 13,          /* the steps of the passed games */
    BGX_ARENA_MATCH_WINS_A_SEAT0 = 14,        /* matches won by A in which A sat as PLAYER1 in the first game */
    BGX_ARENA_MATCH_MATCHES_SEAT0 = 15        /* matches in which A sat as PLAYER1 in the first game */
};
int bgx_arena_match_begin(int32_t n, int32_t length, uint8_t* away_dev, uint8_t* craw_dev, uint8_t* cube_dev,
                          int32_t* plies_dev, int32_t* matches_done_dev, uint8_t* seat0_dev, uint8_t* retire_dev,
                          int64_t* match_tally_dev, void* stream);
int bgx_arena_match_sel(const uint8_t* records_dev, const uint8_t* sel_a_dev, const uint8_t* sel_b_dev,
                        const int32_t* plies_dev, const uint8_t* cube_dev, const uint8_t* away_dev,
                        const uint8_t* craw_dev, int32_t n, uint8_t* dsel_a_out, uint8_t* dsel_b_out, void* stream);
int bgx_arena_match_offer(const uint8_t* records_dev, const uint8_t* sel_a_dev, const uint8_t* sel_b_dev,
                          const uint8_t* dsel_a_dev, const uint8_t* dsel_b_dev, const float* eq_a_dev,
                          const float* eq_b_dev, bgx_match_rule rule_a, bgx_match_rule rule_b, const float* met_dev,
                          const float* pc_dev, int32_t length, const int32_t* plies_dev, const uint8_t* cube_dev,
                          const uint8_t* away_dev, const uint8_t* craw_dev, int32_t n, uint8_t* off_a_out,
                          uint8_t* off_b_out, int64_t* match_tally_dev, void* stream);
int bgx_arena_match_respond(const uint8_t* records_dev, const uint8_t* off_a_dev, const uint8_t* off_b_dev,
                            const float* eq_a_dev, const float* eq_b_dev, bgx_match_rule rule_a, bgx_match_rule rule_b,
                            const float* met_dev, const float* pc_dev, int32_t length, int32_t n,
                            int32_t games_per_lane, int32_t matches_per_lane, uint8_t* cube_dev, int32_t* plies_dev,
                            uint8_t* away_dev, uint8_t* craw_dev, int32_t* matches_done_dev, uint8_t* seat0_dev,
                            int32_t* games_done_dev, uint8_t* sel_a_dev, uint8_t* sel_b_dev, int64_t* tally_dev,
                            int64_t* match_tally_dev, uint8_t* reset_mask_out, void* stream);
int bgx_arena_match_flush(const uint8_t* sel_a_dev, const uint8_t* sel_b_dev, const uint8_t* done_dev,
                          const int32_t* info_dev, const int32_t* games_done_dev, int32_t n, int32_t length,
                          int32_t matches_per_lane, uint8_t* cube_dev, int32_t* plies_dev, uint8_t* away_dev,
                          uint8_t* craw_dev, int32_t* matches_done_dev, uint8_t* seat0_dev, uint8_t* retire_dev,
                          int64_t* match_tally_dev, void* stream);
int bgx_arena_match_retire(int32_t n, int32_t games_per_lane, uint8_t* retire_dev, int32_t* games_done_dev,
                           uint8_t* sel_a_dev, uint8_t* sel_b_dev, int64_t* tally_dev, void* stream);

/* ---- match-score rollouts: position rollouts at a fixed match score, the result a histogram of
 * outcomes (csrc/bg_match_rollout.h; bgx/match.py, bgx/rollout.py; no counterpart
 * in the reference) ----
 * A match rollout plays single games from the lanes' start records at a fixed score; it never
 * carries a score from game to game.  Beside the state of bgx_rollout_begin / bgx_rollout_advance
 * the caller owns, per tally group: away uint8[n_groups, 2], the points PLAYER1 (mover byte 0)
 * and PLAYER2 still need, each in 1..L (L = length in 1..25); craw uint8[n_groups], 0 before the
 * Crawford game, 1 the Crawford game, 2 after it; per lane: cube0 uint8[n], the cube byte every
 * game on the lane starts with, and cube uint8[n], the current one, both read with cap 10
 * (bgx_rollout_cube_begin with cap 10 initialises cube from cube0); dsel and reset_mask uint8[n];
 * value float[n], the value of the side on roll by the rule's own source; and match_hist
 * int64[n_groups][96] (bgx_rollout_match_field), zeroed by the caller.  The tables met and pc,
 * met_after, the rule bgx_match_rule, ND / DT / DP, access, offer and answer are those of the
 * block above, with one rule for both sides: the side on roll (record byte 52 = m) needs x =
 * away[g][m], the other y = away[g][1 - m], and the offer and the answer are made on the same
 * value[i], the answer with the shares swapped.  Indices are total as in met_after: a hand-set
 * score cannot read outside the tables (x = 0 gives no access).
 * The decision of a step: without access none.  With access the side on roll doubles iff the offer
 * rule holds; then the other side passes iff the answer rule holds, else it takes: k += 1, owner =
 * 2 - m.  A pass ends the game: the doubler wins 2^k (k before the double).  A played-out game
 * gives its winner s 2^k, s = info's game_score in 1..3, with no Jacoby rule.  A NaN value never
 * doubles and never passes.
 * The histogram: bins 0..87, index won * 44 + kind * 11 + k, won = 1 when the start record's mover
 * (starts byte 52) won the game, kind 0 a pass and 1 / 2 / 3 the played-out score, k in 0..10 the
 * cube at the end (before the double for a pass).  Entries 88..93 are the sums below; 94 and 95
 * stay zero.  The host turns the bins into the match-winning chance with met_after.
 * Per step: match_sel; the value on dsel; match_decide; bgx_reset with the mask; the player's act;
 * bgx_arena_merge; bgx_step; match_flush; bgx_rollout_advance.
 * bgx_rollout_match_sel: dsel_out[i] = 1 when sel[i] != 0, the group is valid and the side on
 * roll has access by the lane's record, plies[i], cube[i] and its group's score; else 0.
 * bgx_rollout_match_decide: on a lane with dsel[i] != 0 and a valid group, access tested again
 * (with sel[i] as the lane's activity): the decision above on value[i].  A double counts
 * DOUBLES_START when the side on roll is the start record's mover, else DOUBLES_OTHER.  A take
 * turns the cube.  A pass adds 1 to its bin, GAMES and PASS_GAMES, k to LOG2 and plies[i] to
 * PASS_PLIES; games_done[i] += 1, plies[i] = 0, cube[i] = cube0[i]; the lane's last game: sel[i] =
 * 0 and active drops; reset_mask_out[i] = 1.  Every other lane gets reset_mask_out[i] = 0.
 * bgx_rollout_match_flush: after bgx_step and BEFORE bgx_rollout_advance.  A done with a winner on
 * a lane with sel[i] != 0 and a valid group adds 1 to its bin at the cube's k and to GAMES, and k
 * to LOG2.  Any done puts cube0[i] back.
 * bgx_match_decision: the static answer per lane, no rollout state: records uint8[n, 64], cube
 * uint8[n], away uint8[n, 2] (by player), craw uint8[n], value float[n].  values_out float[n, 3] =
 * ND, DT, DP of the side on roll; flags_out uint8[n]: bit 0 access (without the plies > 0 term),
 * bit 1 it offers (access and the offer rule), bit 2 the other side passes a double (the answer
 * rule, whether or not one is offered), bit 3 too good (ND > DP).  A NaN value gives NaN for ND
 * and DT and clears bits 1 to 3.
 * All sums are integers, hence run-to-run identical.  Plain kernels, one thread per lane, no
 * allocation and no synchronisation: graph-capturable.  BGX_EINVAL for a NULL pointer, n <= 0,
 * n_groups <= 0, games_per_lane < 0, length outside 1..25, a NaN scale, or window or a gammon
 * share outside [0, 1] (a NaN included). */
#define BGX_ROLLOUT_MATCH_BINS 88
#define BGX_ROLLOUT_MATCH_ROW 96
enum bgx_rollout_match_field {
    BGX_ROLLOUT_MATCH_GAMES = 88,          /* games that ended, played out or passed: the sum of the bins */
    BGX_ROLLOUT_MATCH_PASS_GAMES = 89,     /* games ended by a passed double */
    BGX_ROLLOUT_MATCH_DOUBLES_START = 90,  /* doubles offered by the start mover's side */
    BGX_ROLLOUT_MATCH_DOUBLES_OTHER = 91,  /* doubles offered by the other side */
    BGX_ROLLOUT_MATCH_PASS_PLIES = 92,     /* the steps of the passed games */
    BGX_ROLLOUT_MATCH_LOG2 = 93            /* sum of k at the game's end */
};
int bgx_rollout_match_sel(const uint8_t* records_dev, const int32_t* group_dev, int32_t n_groups,
                          const int32_t* plies_dev, const uint8_t* sel_dev, const uint8_t* cube_dev,
                          const uint8_t* away_dev, const uint8_t* craw_dev, int32_t n, uint8_t* dsel_out, void* stream);
int bgx_rollout_match_decide(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* group_dev,
                             const uint8_t* dsel_dev, const float* value_dev, int32_t n, int32_t n_groups,
                             int32_t games_per_lane, bgx_match_rule rule, const float* met_dev, const float* pc_dev,
                             int32_t length, const uint8_t* away_dev, const uint8_t* craw_dev, const uint8_t* cube0_dev,
                             uint8_t* cube_dev, int32_t* games_done_dev, int32_t* plies_dev, uint8_t* sel_dev,
                             int64_t* match_hist_dev, int64_t* active_dev, uint8_t* reset_mask_out, void* stream);
int bgx_rollout_match_flush(const uint8_t* starts_dev, const int32_t* group_dev, const uint8_t* sel_dev,
                            const uint8_t* done_dev, const int32_t* info_dev, int32_t n, int32_t n_groups,
                            const uint8_t* cube0_dev, uint8_t* cube_dev, int64_t* match_hist_dev, void* stream);
int bgx_match_decision(const uint8_t* records_dev, const uint8_t* cube_dev, const uint8_t* away_dev,
                       const uint8_t* craw_dev, const float* value_dev, int32_t n, bgx_match_rule rule,
                       const float* met_dev, const float* pc_dev, int32_t length, float* values_out, uint8_t* flags_out,
                       void* stream);

/* ---- truncated position rollouts (csrc/bg_trunc.h; bgx/rollout.py; no
 * counterpart in the reference) ----
 * A game that has run `horizon` plies without ending stops there and is scored with a value of
 * the position it reached.  Beside the state of bgx_rollout_begin / bgx_rollout_advance: tsel
 * uint8[n], value float[n] (the caller's: bgx_value_lanes or bgx_roll_luck's mean_out with tsel
 * as the lane selection, or any other source), trunc_tally int64[n_groups][7]
 * (bgx_rollout_trunc_field), zeroed by the caller, and reset_mask_out uint8[n].  Per step:
 * [bgx_roll_luck, bgx_rollout_luck_add,] the players' act, bgx_step, [bgx_rollout_luck_flush,]
 * bgx_rollout_advance, trunc_sel, the value of the tsel lanes, trunc_cut, bgx_reset with the
 * mask.  After advance a truncated game's luck sum is complete: the roll now in the record is
 * added only at the next step.
 * bgx_rollout_trunc_sel: tsel_out[i] = 1 when sel[i] != 0, the group is valid, the record is not
 * game_over (byte 55) and plies[i] >= horizon; else 0.  count_inout (int64[1], may be NULL) is
 * increased by the number of lanes set.  BGX_EINVAL for horizon < 1.
 * bgx_rollout_trunc_cut: for a lane with tsel[i] != 0 and a valid group, v = value[i] = the
 * equity of the record's mover (byte 52):
 *   e = scale * v in fp32 (one product);  e = 0 for a NaN, else clamped to [-3, 3];
 *   y = e when the record's mover is the start record's mover, else -e;
 *   Vq = llrintf(y * 65536.0f)                                    (|Vq| <= 196608);
 *   row group[i]: TRUNC_GAMES += 1, TRUNC_PLIES += plies[i], TRUNC_V += Vq, TRUNC_V2 += Vq * Vq;
 *   with lane_luck (float[n], may be NULL): Lq as bgx_rollout_luck_flush defines it
 *   (llrintf(lane_luck[i] * 65536.0f) clamped to +-2^21, 0 when not finite), TRUNC_LUCK += Lq,
 *   TRUNC_LUCK2 += Lq * Lq, TRUNC_VLUCK += Vq * Lq (units of 2^-32; at most 2^39 each, so a row
 *   holds 2^24 games), lane_luck[i] = 0;
 *   games_done[i] += 1, plies[i] = 0; the lane's last game: sel[i] = 0 and active drops;
 *   reset_mask_out[i] = 1.
 * Every other lane gets reset_mask_out[i] = 0 and is otherwise untouched.  The caller then runs
 * bgx_reset with the mask, which gives each truncated lane its start record again.  The sums
 * are integers: run-to-run identical.  Plain kernels, one thread per lane, no allocation and no
 * synchronisation: graph-capturable.  BGX_EINVAL for n <= 0, n_groups <= 0, games_per_lane < 0,
 * a NaN scale or a NULL pointer (other than count_inout and lane_luck). */
enum bgx_rollout_trunc_field {
    BGX_ROLLOUT_TRUNC_GAMES = 0,      /* truncated games */
    BGX_ROLLOUT_TRUNC_PLIES = 1,      /* their steps */
    BGX_ROLLOUT_TRUNC_V = 2,          /* sum of Vq (2^-16 points, from the start mover's side) */
    BGX_ROLLOUT_TRUNC_V2 = 3,         /* sum of Vq^2 (2^-32) */
    BGX_ROLLOUT_TRUNC_LUCK = 4,       /* sum of Lq (2^-16) */
    BGX_ROLLOUT_TRUNC_LUCK2 = 5,      /* sum of Lq^2 (2^-32) */
    BGX_ROLLOUT_TRUNC_VLUCK = 6       /* sum of Vq * Lq (2^-32) */
};
int bgx_rollout_trunc_sel(const uint8_t* records_dev, const int32_t* group_dev, int32_t n, int32_t n_groups,
                          int32_t horizon, const int32_t* plies_dev, const uint8_t* sel_dev, uint8_t* tsel_out,
                          int64_t* count_inout_or_null, void* stream);
int bgx_rollout_trunc_cut(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* group_dev,
                          const uint8_t* tsel_dev, const float* value_dev, float scale, int32_t n,
                          int32_t n_groups, int32_t games_per_lane, int32_t* games_done_dev, int32_t* plies_dev,
                          uint8_t* sel_dev, float* lane_luck_or_null, int64_t* trunc_tally_dev,
                          int64_t* active_dev, uint8_t* reset_mask_out, void* stream);

/* ---- cubeful exact bearoff table (csrc/bg_bearoff_cube.h; bgx/bearoff.py, bgx/cube.py,
 * bgx/rollout.py; no counterpart in the reference) ----
 * The money-play equity, with an unlimited doubling cube, of every race of the two-sided table,
 * in units of the current cube and from the view of the side on roll with configuration a
 * against b.  No gammons: both sides have checkers off.  Three cube states as the side on roll
 * sees them -- cen (centred), own (it owns the cube), opp (the opponent owns it) -- and
 *   child(cen) = cen, child(own) = opp, child(opp) = own   (the state as the next roller sees it)
 *   ND_s[a][b] = sum over r = 0..20, from 0.0f, of p_r * max over a' in succ(a, r) of
 *                (a' empty ? 1.0f : -E_child(s)[b][a'])
 *   E_opp[a][b] = ND_opp[a][b];  DT[a][b] = 2.0f * E_opp[a][b]
 *   E_s[a][b] = max(ND_s[a][b], min(DT[a][b], 1.0f))   for s = cen, own
 *   E_s[a][empty] = ND_s[a][empty] = -1;  E_s[empty][b] = ND_s[empty][b] = +1 (b not empty)
 * with p_r, the roll order and succ those of the two-sided table; every product and sum is
 * rounded to fp32 once, with no fma, so a numpy float32 loop gives the same bits.  The roller
 * doubles iff min(DT, 1) > ND_s (a tie is no double), the opponent takes iff DT <= 1.
 * bgx_bearoff_cube_create builds it from an existing database `db` (whose W, configs and
 * successor sets it reads, and which must outlive it) on `stream` of db's device, one launch per
 * total pip count, and synchronises the stream.  bgx_bearoff_cube_buffers: equity float[3][n][n]
 * in the order cen, own, opp, nd float[2][n][n] in the order cen, own, configs = db's.
 * bgx_bearoff_cube_destroy synchronises the device.
 *
 * bgx_bearoff_cube_lookup: one thread per 64-byte record (16-byte aligned), bgx_bearoff_lookup's
 * record test and in_db_out.  cube_dev uint8[n] (NULL: centred at 1 on every lane) is read as the
 * cube kernels read it (k as min(k, cap), owner 3 as 0; cap in 0..10).  With m the record's
 * mover: k >= cap is the dead state, owner 0 cen, owner m + 1 own, otherwise opp.  For a record
 * in the table values_out float[n][4] (16-byte aligned, may be NULL) receives
 *   [0] nd, the mover's equity if it does not double now (ND_s; E_opp in opp),
 *   [1] DT,  [2] e = max(nd, min(DT, 1)) with access (cen, own) and nd without,
 *   [3] the cubeless 2 W - 1 (fp32: the product, then the difference);  dead: nd = e = [3],
 * and flags_out uint8[n] (may be NULL) bit 0: the mover may double, bit 1: it doubles, bit 2:
 * the opponent takes (DT <= 1), bit 3: the cube is dead.  Other records: values not written,
 * flags 0.  The table assumes an unlimited cube below the cap: that the cap could be reached
 * deeper inside the table is ignored.  No allocation, no synchronisation: graph-capturable.
 *
 * bgx_rollout_cube_bearoff_cut: bgx_rollout_bearoff_cut for cubeful rollouts.  Call it once after
 * bgx_rollout_begin and bgx_rollout_cube_begin and after every bgx_rollout_advance; the caller
 * runs the masked bgx_reset after it.  cube_cut_tally int64[n_groups][6]
 * (bgx_rollout_cube_cut_field) is zeroed by the caller.  A lane with sel[i] != 0, a valid group
 * and a record in the table, k and the state read from cube[i] as in the lookup:
 *   v = nd when plies[i] == 0 (no cube action on a game's first ply: a start record is the
 *       position after the decision), else e;
 *   q = v when the record's mover is the start record's mover, else -v;
 *   Qq = llrintf(q * 1048576.0f) clamped to +-2^20;  Yq = Qq * 2^k  (|Yq| <= 2^30);
 *   row group[i]: GAMES += 1, PLIES += plies[i], Y += Yq, Y2_LO += Yq^2 & (2^30 - 1),
 *   Y2_HI += Yq^2 >> 30, LOG2 += k;
 *   games_done[i] += 1, plies[i] = 0; the lane's last game: sel[i] = 0 and active drops;
 *   cube[i] = cube0[i]; reset_mask_out[i] = 1.
 * Every other lane gets reset_mask_out[i] = 0.  The sums are integers: run-to-run identical; a
 * row holds 2^33 cut games.  No allocation, no synchronisation: graph-capturable.  BGX_EINVAL
 * for what bgx_rollout_bearoff_cut and the cube kernels reject. */
typedef struct bgx_bearoff_cube bgx_bearoff_cube;
typedef struct {
    const float* equity;       /* [3][n][n] cen, own, opp */
    const float* nd;           /* [2][n][n] cen, own */
    const int8_t* configs;
    int32_t n, max_checkers;
} bgx_bearoff_cube_buffers;
enum bgx_rollout_cube_cut_field {
    BGX_ROLLOUT_CUBE_CUT_GAMES = 0,   /* cut games */
    BGX_ROLLOUT_CUBE_CUT_PLIES = 1,   /* their steps */
    BGX_ROLLOUT_CUBE_CUT_Y = 2,       /* sum of Yq (2^-20 points, from the start mover's side) */
    BGX_ROLLOUT_CUBE_CUT_Y2_LO = 3,   /* sum of Yq^2 & (2^30 - 1) */
    BGX_ROLLOUT_CUBE_CUT_Y2_HI = 4,   /* sum of Yq^2 >> 30: sum Yq^2 = Y2_HI 2^30 + Y2_LO (2^-40) */
    BGX_ROLLOUT_CUBE_CUT_LOG2 = 5     /* sum of k at the cut */
};
int bgx_bearoff_cube_create(bgx_bearoff* db, void* stream, bgx_bearoff_cube** out);
int bgx_bearoff_cube_buffers_get(bgx_bearoff_cube* cdb, bgx_bearoff_cube_buffers* out);
int bgx_bearoff_cube_destroy(bgx_bearoff_cube* cdb);
int bgx_bearoff_cube_lookup(const bgx_bearoff_cube* cdb, const uint8_t* records_dev, const uint8_t* cube_dev, int32_t n,
                            int32_t cap, uint8_t* in_db_out, float* values_out, uint8_t* flags_out, void* stream);
int bgx_rollout_cube_bearoff_cut(const bgx_bearoff_cube* cdb, const uint8_t* records_dev, const uint8_t* starts_dev,
                                 const int32_t* group_dev, int32_t n, int32_t n_groups, int32_t games_per_lane,
                                 int32_t* games_done_dev, int32_t* plies_dev, uint8_t* sel_dev,
                                 int64_t* cube_cut_tally_dev, int64_t* active_dev, uint8_t* reset_mask_out, int32_t cap,
                                 const uint8_t* cube0_dev, uint8_t* cube_dev, void* stream);

/* ---- truncated cubeful rollouts and the static cube evaluator (csrc/bg_cube_trunc.h;
 * bgx/cube.py, bgx/rollout.py; no counterpart in the reference) ----
 * The value of a position with a cube on it from one cubeless value v of the side on roll, by
 * Janowski's interpolation between the dead-cube and the live-cube equity.  Everything is in
 * units of the current cube and from the view of the side on roll.  bgx_cube_life: cube_life x in
 * [0, 1], win_value W and loss_value L, the mean points of a won / lost game, in [1, 3].  In
 * fp32, every operation rounded once, no fma (a numpy float32 restatement gives the same bits):
 *   c = scale * v;  c = 0 for a NaN, else clamped to [-L, W]      the dead-cube equity
 *   p = (c + L) / (W + L)                                         the inferred win probability
 *   D = W + L + 0.5f;  TP = (L - 0.5f) / D;  CP = (L + 1.0f) / D  live-cube take and cash points
 *   seg(p; p0, y0, p1, y1) = y0 + (p - p0) * ((y1 - y0) / (p1 - p0))
 *   live_cen(p) = p < TP ? seg(p; 0,-L, TP,-1) : p < CP ? seg(p; TP,-1, CP,1) : seg(p; CP,1, 1,W)
 *   live_own(p) = p < CP ? seg(p; 0,-L, CP,1) : seg(p; CP,1, 1,W)
 *   live_opp(p) = p < TP ? seg(p; 0,-L, TP,-1) : seg(p; TP,-1, 1,W)
 *   E_s(p) = (1 - x) * c + x * live_s(p)                          s = cen, own, opp
 * With jacoby != 0, E_cen is formed with W = L = 1 (c' = 2 p - 1, TP = 0.2, CP = 0.8; p as
 * above).  The cube byte is read as the cube kernels read it (k as min(k, cap), owner 3 as 0);
 * with m the record's mover (byte 52): k >= cap is the dead state (E = c), owner 0 cen, owner
 * m + 1 own, otherwise opp.  The four values and the flags are bgx_bearoff_cube_lookup's:
 *   [0] nd = E_s(p);  [1] DT = 2 E_opp(p), or 2 c when k + 1 >= cap (never the Jacoby form);
 *   [2] e = max(nd, min(DT, 1)) where the mover may double (cen or own, k < cap), else nd;
 *   [3] c;  flags bit 0: the mover may double, bit 1: it doubles (min(DT, 1) > nd; a tie is no
 *   double), bit 2: the opponent takes (DT <= 1), bit 3: the cube is dead.
 * bgx_cube_janowski: one thread per 64-byte record.  cube_dev uint8[n] (NULL: centred at 1 on
 * every lane), value float[n], sel uint8[n] (NULL: every lane).  A selected record that is not
 * game_over (byte 55) writes values_out float[n][4] (16-byte aligned, may be NULL) and its flags
 * to flags_out uint8[n] (may be NULL); every other lane gets flags 0 and its values are not
 * written.
 * bgx_rollout_cube_trunc_cut: bgx_rollout_trunc_cut for cubeful rollouts, after
 * bgx_rollout_advance and bgx_rollout_trunc_sel (tsel) and the value of the tsel lanes; the caller
 * runs the masked bgx_reset after it.  cube_trunc_tally int64[n_groups][6]
 * (bgx_rollout_cube_trunc_field) is zeroed by the caller.  A lane with tsel[i] != 0 and a valid
 * group, k and the state read from cube[i]:
 *   q = e when the record's mover is the start record's mover, else -e (e and not nd: the mover
 *       has not yet taken this ply's cube decision);
 *   Qq = llrintf(q * 65536.0f) clamped to +-196608;  Yq = Qq * 2^k  (|Yq| <= 3 * 2^26);
 *   row group[i]: GAMES += 1, PLIES += plies[i], Y += Yq, Y2_LO += Yq^2 & (2^30 - 1),
 *   Y2_HI += Yq^2 >> 30, LOG2 += k;
 *   games_done[i] += 1, plies[i] = 0; the lane's last game: sel[i] = 0 and active drops;
 *   cube[i] = cube0[i]; reset_mask_out[i] = 1.
 * Every other lane gets reset_mask_out[i] = 0 and is otherwise untouched.  The unit is
 * bgx_rollout_trunc_cut's 2^-16 points, so a dead-cube run equals a plain truncated run integer
 * for integer.  The sums are integers: run-to-run identical.  Plain kernels, one thread per lane,
 * no allocation and no synchronisation: graph-capturable.  BGX_EINVAL for what
 * bgx_rollout_trunc_cut and the cube kernels reject (n <= 0, n_groups <= 0, games_per_lane < 0, a
 * NaN scale, cap outside 0..10, a NULL pointer other than those named), a misaligned values_out,
 * and a cube_life, win_value or loss_value that is NaN or outside its range. */
typedef struct {
    float cube_life;           /* x in [0, 1]: 0 = dead cube, 1 = live cube */
    float win_value;           /* W in [1, 3]: mean points of a won game */
    float loss_value;          /* L in [1, 3]: mean points of a lost game */
} bgx_cube_life;
enum bgx_rollout_cube_trunc_field {
    BGX_ROLLOUT_CUBE_TRUNC_GAMES = 0,   /* truncated games */
    BGX_ROLLOUT_CUBE_TRUNC_PLIES = 1,   /* their steps */
    BGX_ROLLOUT_CUBE_TRUNC_Y = 2,       /* sum of Yq (2^-16 points, from the start mover's side) */
    BGX_ROLLOUT_CUBE_TRUNC_Y2_LO = 3,   /* sum of Yq^2 & (2^30 - 1) */
    BGX_ROLLOUT_CUBE_TRUNC_Y2_HI = 4,   /* sum of Yq^2 >> 30: sum Yq^2 = Y2_HI 2^30 + Y2_LO (2^-32) */
    BGX_ROLLOUT_CUBE_TRUNC_LOG2 = 5     /* sum of k at the truncation */
};
int bgx_cube_janowski(const uint8_t* records_dev, const uint8_t* cube_dev_or_null, const float* value_dev, int32_t n,
                      float scale, bgx_cube_life life, int32_t cap, int32_t jacoby, const uint8_t* sel_or_null,
                      float* values_out, uint8_t* flags_out, void* stream);
int bgx_rollout_cube_trunc_cut(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* group_dev,
                               const uint8_t* tsel_dev, const float* value_dev, float scale, bgx_cube_life life,
                               int32_t n, int32_t n_groups, int32_t games_per_lane, int32_t* games_done_dev,
                               int32_t* plies_dev, uint8_t* sel_dev, int64_t* cube_trunc_tally_dev, int64_t* active_dev,
                               uint8_t* reset_mask_out, int32_t cap, int32_t jacoby, const uint8_t* cube0_dev,
                               uint8_t* cube_dev, void* stream);

/* ---- luck of cubeful rollouts (csrc/bg_cube_luck.h; bgx/cube.py, bgx/rollout.py; DESIGN.md §18;
 * no counterpart in the reference) ----
 * The luck adjustment of bgx_rollout_luck_* for games with a cube.  Everything per roll is in
 * units of the lane's current cube and from the view of the side on roll m (record byte 52).
 * bgx_cube_roll_luck: one thread per 64-byte record, 256 per block.  values21 float[n][21] =
 * bgx_roll_values' v_r; cube uint8[n] (NULL: centred at 1 everywhere), read as every cube kernel
 * reads it; sel uint8[n] (NULL: every lane).  After m plays roll r its opponent is on roll with
 * the same cube, before its own cube decision, so with the rule of bgx_cube_janowski
 *   g_r  = -e  of  (cube byte, cap, side on roll 1 - m, scale, value -v_r, life, jacoby)
 *   mean = fma(p_20, g_20, ... fma(p_0, g_0, 0)) in fp32, p_r = 1/36 for doubles, else 2/36
 *   luck = g_(the record's roll, bytes 53, 54) - mean in fp32   (0 when they hold no roll)
 * (the two negations are exact).  A selected record that is not game_over writes luck_out[i]
 * and, when it is given, mean_out[i]; other lanes are not written.  g is a fixed function of the
 * position after the roll and of the cube, which is known before the roll, so the luck has mean
 * zero given the history whatever the net, the life or the scale.  BGX_EINVAL for n <= 0, a NULL
 * records, values21 or luck_out, cap outside 0..10, a life outside its ranges or a NaN scale.
 *
 * The bookkeeping, beside bgx_rollout_cube_*'s state: lane_luck float[n] (the running sum of the
 * lane's current game, in POINTS) and cube_luck_tally int64[n_groups][5]
 * (bgx_rollout_cube_luck_field), both zeroed by the caller.  A game's luck L is the fp32 sum in
 * step order of s * 2^k * luck, s = +1 when the step's mover is the start record's mover, else
 * -1, k the lane's cube AFTER that step's cube decision (the product with 2^k is exact).  When
 * the game is booked, Lq = llrintf(L * 65536) clamped to +-2^31, 0 when not finite, and with y the
 * game's cubeful result in points from the start mover's side, row group[i] gets
 *   LUCK += Lq, LUCK2_LO += Lq^2 & (2^30 - 1), LUCK2_HI += Lq^2 >> 30, YLUCK += y * Lq,
 *   LUCK_GAMES += 1.
 * |y| <= 3 * 2^10, so |y Lq| < 2^43 and Lq^2 <= 2^62: a row holds 2^20 games at the clamp.
 * bgx_rollout_cube_luck_pass: BEFORE bgx_rollout_cube_decide, with the same dsel, equity, rule
 * and cube.  It evaluates the decision exactly as that call will; a lane with dsel[i] != 0 and a
 * valid group whose double is passed books its game against y = +-2^k (the doubler wins) and
 * gets lane_luck[i] = 0.  Nothing else is written: the decision itself stays with cube_decide.
 * bgx_rollout_cube_luck_add: after cube_decide and the masked bgx_reset, before the players act,
 * with luck_dev = bgx_cube_roll_luck's luck_out for the lanes as they stand.  Every lane with
 * sel[i] != 0, except bgx_rollout_luck_add's first step of a game whose start record fixed the
 * roll: lane_luck[i] += records[i][52] == starts[i][52] ? ldexp(luck[i], k) : -ldexp(luck[i], k).
 * bgx_rollout_cube_luck_flush: after bgx_step and BEFORE bgx_rollout_cube_flush (which puts the
 * starting cube back), with the step's done and info.  A lane with sel[i] != 0, a valid group
 * and a game that bgx_rollout_advance counts books it against y = +-(score << k), score 1 under
 * the Jacoby rule while k = 0 (bgx_rollout_cube_flush's result), and gets lane_luck[i] = 0; any
 * other done of a selected lane only zeroes lane_luck[i].
 * LUCK_GAMES equals BGX_ROLLOUT_CUBE_GAMES of the row.  One thread per lane, the sums combined
 * per wave and group before the 64-bit atomics; integers, so run-to-run identical.  No
 * allocation and no synchronisation: graph-capturable.  BGX_EINVAL for n <= 0, n_groups <= 0,
 * cap outside 0..10, a rule bgx_rollout_cube_decide rejects, or a NULL pointer. */
enum bgx_rollout_cube_luck_field {
    BGX_ROLLOUT_CUBE_LUCK = 0,         /* sum of Lq (2^-16 points) */
    BGX_ROLLOUT_CUBE_LUCK2_LO = 1,     /* sum of Lq^2 & (2^30 - 1) */
    BGX_ROLLOUT_CUBE_LUCK2_HI = 2,     /* sum of Lq^2 >> 30: sum Lq^2 = LUCK2_HI 2^30 + LUCK2_LO (2^-32) */
    BGX_ROLLOUT_CUBE_YLUCK = 3,        /* sum of y * Lq (2^-16), y in points */
    BGX_ROLLOUT_CUBE_LUCK_GAMES = 4    /* games booked: equals BGX_ROLLOUT_CUBE_GAMES of the row */
};
int bgx_cube_roll_luck(const uint8_t* records_dev, const uint8_t* cube_dev_or_null, const float* values21_dev,
                       int32_t n, float scale, bgx_cube_life life, int32_t cap, int32_t jacoby,
                       const uint8_t* sel_or_null, float* luck_out, float* mean_out_or_null, void* stream);
int bgx_rollout_cube_luck_add(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* plies_dev,
                              const uint8_t* sel_dev, const uint8_t* cube_dev, const float* luck_dev, int32_t n,
                              int32_t cap, float* lane_luck_dev, void* stream);
int bgx_rollout_cube_luck_pass(const uint8_t* records_dev, const uint8_t* starts_dev, const int32_t* group_dev,
                               const uint8_t* dsel_dev, const float* equity_dev, int32_t n, int32_t n_groups,
                               bgx_cube_rule rule, const uint8_t* cube_dev, float* lane_luck_dev,
                               int64_t* cube_luck_tally_dev, void* stream);
int bgx_rollout_cube_luck_flush(const uint8_t* starts_dev, const int32_t* group_dev, const uint8_t* sel_dev,
                                const uint8_t* done_dev, const int32_t* info_dev, int32_t n, int32_t n_groups,
                                int32_t cap, int32_t jacoby, const uint8_t* cube_dev, float* lane_luck_dev,
                                int64_t* cube_luck_tally_dev, void* stream);

/* ---- luck of the arena (csrc/bg_arena_luck.h; bgx/arena.py; no counterpart in
 * the reference) ----
 * The luck adjustment of bgx_rollout_luck_* for the cubeless head-to-head arena, beside the state
 * of bgx_arena_begin / bgx_arena_advance.  Two things differ from a rollout.  The sign: there is
 * no start record, a game's luck is kept from A's side, so a roll's luck counts + where A is on
 * move (sel_a) and - where B is (sel_b).  The opening roll: an arena game begins with the engine's
 * standard reset, whose first roll is drawn with doubles rejected, so on a game's first ply the
 * mean is taken over the 15 non-doubles at 1/15 each, not over the 21 rolls at 1/36 and 2/36.
 * State, the caller's: lane_luck float[n] (the running sum of the lane's current game), fresh
 * uint8[n] (the lane's record holds an opening roll) and luck_tally int64[8]
 * (bgx_arena_luck_field; entries 5..7 stay zero).
 * bgx_arena_luck_begin: once after bgx_arena_begin: lane_luck = 0, fresh = 1, luck_tally = 0.
 * bgx_arena_luck_add: before the players act, with values21 float[n][21] = bgx_roll_values' v_r
 * of the lanes with sel_a | sel_b.  Every lane with sel_a[i] | sel_b[i] whose record is not
 * game_over, with (d0, d1) the record's roll (bytes 53, 54):
 *   fresh[i] == 0: mean = fma(p_20, v_20, ... fma(p_0, v_0, 0)), p_r = 1/36 for doubles, else 2/36
 *                  (bgx_roll_luck's mean_out and luck_out bit for bit)
 *   fresh[i] != 0: mean = fma(1/15, v_r, mean) over the 15 non-doubles, r ascending, from 0; the
 *                  doubles' values are not read into the chain
 *   luck = v_(the record's roll) - mean in fp32   (0 when the bytes hold no roll, and 0 for a
 *          double while fresh: it cannot have been drawn)
 *   lane_luck[i] += sel_a[i] ? luck : -luck (one fp32 add), fresh[i] = 0,
 * and luck_out[i] = luck (the mover's view), mean_out[i] = mean where they are given.  No other
 * lane is written.  Either mean is the expectation of v under the distribution the roll was drawn
 * from, given the position and the mover, so the luck has mean zero given the history.
 * bgx_arena_luck_flush: after bgx_step and BEFORE bgx_arena_advance (games_done and the
 * selections are still the step's), with the step's done and info.  A lane with sel_a | sel_b and
 * games_done < games_per_lane whose game bgx_arena_advance will count (done, a winner) books it:
 * res = A's result as advance books it (+-1 / 2 / 3; 0 points for a score outside 1..3),
 * Lq = llrintf(lane_luck[i] * 65536) clamped to +-2^21 (0 when not finite; round half even:
 * bgx_rollout_luck_flush's), and
 *   LUCK += Lq, LUCK2_LO += Lq^2 & (2^30 - 1), LUCK2_HI += Lq^2 >> 30, RESLUCK += res * Lq,
 *   LUCK_GAMES += 1.
 * Every done of such a lane, counted or not, gets lane_luck[i] = 0 and fresh[i] = 1: the record
 * is the next game's opening already.  LUCK_GAMES equals tally[BGX_ARENA_GAMES].  |Lq| <= 2^21 and
 * |res| <= 3: the sums hold 2^33 games at the clamp.
 * One thread per lane, 256 per block; the sums combined per wave before the 64-bit atomics;
 * integers, so run-to-run identical.  No allocation and no synchronisation: graph-capturable.
 * BGX_EINVAL for n <= 0, games_per_lane < 0 or a NULL pointer other than luck_out / mean_out. */
enum bgx_arena_luck_field {
    BGX_ARENA_LUCK = 0,           /* sum of Lq (2^-16 points), A's view */
    BGX_ARENA_LUCK2_LO = 1,       /* sum of Lq^2 & (2^30 - 1) */
    BGX_ARENA_LUCK2_HI = 2,       /* sum of Lq^2 >> 30: sum Lq^2 = LUCK2_HI 2^30 + LUCK2_LO (2^-32) */
    BGX_ARENA_RESLUCK = 3,        /* sum of res * Lq (2^-16), res = A's points of the game */
    BGX_ARENA_LUCK_GAMES = 4      /* games booked: equals tally[BGX_ARENA_GAMES] */
};
int bgx_arena_luck_begin(int32_t n, float* lane_luck_dev, uint8_t* fresh_dev, int64_t* luck_tally_dev, void* stream);
int bgx_arena_luck_add(const uint8_t* records_dev, const uint8_t* sel_a_dev, const uint8_t* sel_b_dev,
                       const float* values21_dev, int32_t n, float* lane_luck_dev, uint8_t* fresh_dev,
                       float* luck_out_or_null, float* mean_out_or_null, void* stream);
int bgx_arena_luck_flush(const uint8_t* sel_a_dev, const uint8_t* sel_b_dev, const uint8_t* done_dev,
                         const int32_t* info_dev, const int32_t* games_done_dev, int32_t n, int32_t games_per_lane,
                         float* lane_luck_dev, uint8_t* fresh_dev, int64_t* luck_tally_dev, void* stream);

/* ---- PPO update loss head (ppo_agent.py:268-305), fused ----
 * For n rows: masked log-softmax of the logits (dtype 0 = fp32, 1 = fp16, row
 * stride ld_logits; mask from the legal count in bytes 60-61 of each 64-byte
 * lane record: log(1e-45) for illegal actions), ratio = exp(logp[action] -
 * old_logp), clipped surrogate (eps_clip), value MSE, entropy.  Writes the
 * gradients of  policy + c_value * value - c_entropy * entropy  (per-row losses,
 * times grad_scale) with respect to the logits (dlogits, same dtype, row stride
 * ld_dlogits) and the values (dvalues, same dtype), as torch autograd forms them,
 * and adds the sums of the per-row policy loss, squared value error and entropy
 * to sums[0..2] (double, device). */
int bgx_ppo_head(const void* logits_dev, int32_t dtype, int64_t ld_logits, const void* values_dev,
                 const uint8_t* records_dev, const int32_t* actions_dev, const float* old_logp_dev,
                 const float* returns_dev, const float* adv_dev, int32_t n, int32_t n_actions, float eps_clip,
                 float c_value, float c_entropy, float grad_scale, void* dlogits_dev, int64_t ld_dlogits,
                 void* dvalues_dev, double* sums_dev, void* stream);

/* bgx_ppo_head for a [logits | value | 0 ...] layout (one GEMM for both heads,
 * row stride ld_dlogits <= 512): with pad_value_col != 0 the kernel also writes
 * the value gradient into column n_actions of dlogits and zeros up to
 * ld_dlogits; with colsum != NULL (float[BGX_PPO_COLSUM_BLOCKS][512]) each
 * workgroup writes the column sums of the gradient it stored (fp16-rounded
 * when dtype = 1) — the bias gradient, summed over the first dimension by the
 * caller.  dvalues_dev is written as in bgx_ppo_head. */
#define BGX_PPO_COLSUM_BLOCKS 2048
int bgx_ppo_head_ex(const void* logits_dev, int32_t dtype, int64_t ld_logits, const void* values_dev,
                    const uint8_t* records_dev, const int32_t* actions_dev, const float* old_logp_dev,
                    const float* returns_dev, const float* adv_dev, int32_t n, int32_t n_actions, float eps_clip,
                    float c_value, float c_entropy, float grad_scale, void* dlogits_dev, int64_t ld_dlogits,
                    void* dvalues_dev, double* sums_dev, int32_t pad_value_col, float* colsum_dev, void* stream);

/* The fp16 epoch's ReLU backward of fc1 (policy_network.py:70; autograd passes the
 * gradient where relu's output > 0) in place on dh [n][hidden] fp16, given the
 * stored activations h [n][hidden] fp16 (16-byte aligned, hidden % 8 == 0,
 * hidden <= 256), with the bias gradient's partial column sums of the masked dh
 * in colsum[blocks][hidden] (fp32; the caller sums the rows).  The grid is `blocks`
 * workgroups and every one writes its whole colsum row: a block that had no row of
 * dh to walk (n small next to blocks) writes zeros, so colsum needs no clearing. */
int bgx_relu_backward(void* dh, const void* h, int32_t n, int32_t hidden, float* colsum, int32_t blocks,
                      void* stream);

/* The fp16 epoch's fc1 forward from the stored records (ppo_agent.py:274 under
 * autocast, policy_network.py:69-70): h[n][hidden] fp16 = relu(W1h . fp16(x) + b1h)
 * with fp32 accumulation, x = the 198 features of each 64-byte record (off/15
 * rounded to fp16 as autocast's cast rounds it).  W1h [hidden][198] fp16 is packed
 * once per weight update by bgx_fc1_pack into bgx_fc1_packed_size(hidden) bytes
 * (16-byte aligned); b1h [hidden] fp16.  hidden % 4 == 0, hidden <= 128; h 8-byte
 * aligned.  Replaces the materialised feature rows + GEMM for the forward; the
 * weight gradient still reads the encoded features. */
int bgx_fc1_packed_size(int32_t hidden);
int bgx_fc1_pack(const void* w1h_dev, int32_t hidden, void* packed_dev, void* stream);
int bgx_fc1_records(const uint8_t* records_dev, int32_t n, const void* packed_dev, const void* b1h_dev,
                    int32_t hidden, void* h_dev, void* stream);
/* bgx_fc1_records that also raises *hmax2_dev (fp32, device; may be NULL) to the
 * largest |h_row|^2 of its rows (the bound PPOTrainer checks for the fused head's
 * masked-action shortcut, bgx_ppo_rows). */
int bgx_fc1_records_ex(const uint8_t* records_dev, int32_t n, const void* packed_dev, const void* b1h_dev,
                       int32_t hidden, void* h_dev, float* hmax2_dev, void* stream);

/* The fp16 epoch's output layer + loss head without materialised logits
 * (csrc/bg_ppo_fused.hip; replaces, inside ppo_agent.py:268-305 under autocast,
 * the [action_head; value_head] GEMM of policy_network.py:71-75, the loss head of
 * bgx_ppo_head_ex, dh = dy W2h, the ReLU backward and gW2 / gb2 = dy^T [h | 1]).
 * hidden = 128, n_actions = 500; W2h [512][128] fp16 = [action_head.weight;
 * value_head.weight; 0] and b2h [512] fp16 likewise; h [m][128] fp16 = the fc1
 * output (bgx_fc1_records).  perm [m] lists the rows in ascending order of the
 * number of 32-action tiles they need (ceil(cnt / 32), 16 for cnt = 0; any order
 * is correct, sorted is fast); perm = NULL: the rows are already in that order
 * (PPOTrainer gathers them so once per update, and every kernel reads them
 * contiguously).
 * bgx_ppo_rows: per row the loss parts (added to sums[0..2] as bgx_ppo_head),
 * dh [m][128] fp16 = ReLU'(h) * fp16(dy W2h) (original row order), and the row
 * statistics stats [m] (16 B, 16-byte aligned) + info [m] (int32) in perm order
 * for bgx_ppo_gw2; dy_or_null [m][512] fp16 receives dy = [dlogits | dvalue | 0]
 * and z_or_null [m][512] fp16 the logits [y | value] of the 32-column tiles the row's
 * variant computed (other columns untouched) -- both for tests.  row_plan int32[8] = the row tiles (of perm order) [lo, hi) handled by
 * the variants for at most 1, 2, 4 and 16 leading action tiles (every row tile in
 * exactly one range; a tile's count is the largest of its rows').  grid <= 0:
 * persistent grids of 4 workgroups per CU (1 for the 16-tile variant).
 * bgx_ppo_gw2: gw2 [512][128] += dy^T h and gb2 [512] += column sums of dy (fp32),
 * dy recomputed from the statistics; plan int32[33] = task prefix per action tile
 * (17 entries; the tasks of action tile o are the groups of BGX_PPO_GW2_TASK_TILES
 * row tiles, aligned at multiples of it, that hold a row tile >= its start) then the
 * first row tile (of perm order) each action tile needs (16); workspace of
 * bgx_ppo_gw2_workspace(m) bytes. */
#define BGX_PPO_GW2_TASK_TILES 32
int bgx_ppo_rows(const void* h_dev, const int32_t* perm_dev, const uint8_t* records_dev, const int32_t* actions_dev,
                 const float* old_logp_dev, const float* returns_dev, const float* adv_dev, int32_t m, int32_t hidden,
                 int32_t n_actions, const void* w2h_dev, const void* b2h_dev, float eps_clip, float c_value,
                 float c_entropy, float grad_scale, void* dh_dev, void* stats_dev, int32_t* info_dev,
                 double* sums_dev, void* dy_or_null, void* z_or_null, const int32_t* row_plan_dev, int32_t grid,
                 void* stream);
int64_t bgx_ppo_gw2_workspace(int32_t m);
int bgx_ppo_gw2(const void* h_dev, const int32_t* perm_dev, const void* stats_dev, const int32_t* info_dev, int32_t m,
                int32_t hidden, int32_t n_actions, const void* w2h_dev, const void* b2h_dev, float k1,
                const int32_t* plan_dev, float* workspace_dev, float* gw2_dev, float* gb2_dev, void* stream);

/* The fp16 epoch's fc1 weight and bias gradients straight from the records
 * (replaces, inside ppo_agent.py:268-305 under autocast, the weight-gradient GEMM
 * dh^T x of policy_network.py:69-70 over materialised fp16 feature rows):
 * gw1 [128][208] fp32 += dh^T [x | 1 | 0], x = the 198 fp16 features of each
 * 64-byte record (off / 15 rounded as autocast rounds it), column 198 = gb1,
 * 199..207 += 0.  dh [m][128] fp16 (bgx_ppo_rows' output) and records [m][64] in
 * the same row order, both 16-byte aligned; hidden = 128; workspace of
 * bgx_ppo_gw1_workspace(m) bytes (16-byte aligned).  Deterministic (fixed-order
 * partial sums). */
int64_t bgx_ppo_gw1_workspace(int32_t m);
int bgx_ppo_gw1(const void* dh_dev, const uint8_t* records_dev, int32_t m, int32_t hidden, float* workspace_dev,
                float* gw1_dev, void* stream);

/* csrc/bg_returns.hip.  Discounted returns of a [T][B] rollout per game lane (the reference's
 * compute_returns, ppo_agent.py:206-216, restated per lane: R_t = r_t + gamma R_{t+1},
 * reset where done): out [T][B] fp32, the same fp32 roundings as r + gamma * R. */
int bgx_lane_returns(const float* rewards_dev, const uint8_t* dones_dev, int32_t T, int32_t B, float gamma,
                     float* out_dev, void* stream);

/* Zero-sum GAE(lambda) of a [T][B] self-play rollout per game lane (bgx.train.selfplay_gae;
 * DESIGN.md §6 "Self-play returns").  Both players of a game share a lane; records_dev
 * uint8[T][B][64] holds the mover of step t in byte 52, values_dev [T][B] that mover's
 * value.  Walking t = T-1 .. 0 with A_T = 0, cut = done_t, same = (mover_{t+1} == mover_t):
 *   nv = cut ? 0 : (same ? v_{t+1} : -v_{t+1});   na = cut ? 0 : (same ? A_{t+1} : -A_{t+1})
 *   A_t = ((r_t + g nv) - v_t) + gl na;           Ret_t = A_t + v_t
 * in fp32, each product and sum rounded once (no fma); g = fp32(gamma), gl = fp32(g lambda).
 * boot_values_dev [B] and boot_records_dev uint8[B][64] (only byte 52 is read) are v_T and
 * mover_T, the position the rollout stopped in; both NULL: step T-1 is a cut.  adv_dev,
 * ret_dev [T][B] fp32.  sums_dev (fp64[3], may be NULL) receives (sum A, sum A^2, T B):
 * fp64 per-block partials in workspace_dev (bgx_selfplay_gae_workspace(B) bytes; may be
 * NULL with sums_dev NULL) added in a fixed order, identical from run to run.  No host
 * sync, no allocation.  BGX_EINVAL: T <= 0, B <= 0, a NULL required pointer, or exactly one
 * boot pointer. */
int64_t bgx_selfplay_gae_workspace(int32_t B);
int bgx_selfplay_gae(const float* rewards_dev, const uint8_t* dones_dev, const uint8_t* records_dev,
                     const float* values_dev, const float* boot_values_dev, const uint8_t* boot_records_dev,
                     int32_t T, int32_t B, float g, float gl, float* adv_dev, float* ret_dev, double* workspace_dev,
                     double* sums_dev, void* stream);

/* Advantage normalisation in place from sums_dev fp64[3] = (sum, sum of squares, count)
 * read on the device (bgx_selfplay_gae's, all-reduced across ranks where there are several;
 * bgx.ppo.global_normalize's arithmetic): mean = s0 / n and var = (s1 - n mean^2) / (n - 1)
 * in fp64, var clamped at 0, then adv = (adv - fp32(mean)) / (fp32(sqrt(var)) + eps) in fp32. */
int bgx_normalize_adv(float* adv_dev, int64_t n, const double* sums_dev, float eps, void* stream);

/* The fused fp16 PPO epoch's prologue and epilogue (bgx.train._ppo_epoch_amp_fused), one
 * launch each.  bgx_ppo_epoch_prep: from the fp32 parameters (fc1 weight [H][198] and bias,
 * action_head [A][H] and bias, value_head [1][H] and bias) the packed fc1 fragments of
 * fp16(W1) (bgx_fc1_pack's layout, bgx_fc1_packed_size(H) bytes), fp16(b1) [H], W2h =
 * fp16([action_head; value_head; 0]) [512][H], b2h [512], and zeros in the accumulators
 * gw1 [H][208], gw2 [512][H], gb2 [512] and hmax2 [1] (may be NULL), and in bound [2][512]
 * (may be NULL) each action row's |fp16(W)| and |fp16(b)|.  bgx_ppo_epoch_grads:
 * the parameters' gradients from the accumulators times post (fp32): fc1 weight = gw1[:,
 * :198], bias = gw1[:, 198], action_head = gw2[:A], gb2[:A], value_head = gw2[A], gb2[A];
 * with guard_dev (uint8, may be NULL) also guard |= 2 (max_a |W2h[a]| sqrt(hmax2[0]) +
 * max_a |b2h[a]|) > limit over a < A from prep's bound (the fused head's masked-action bound).
 * Loss parts (both may be NULL): prep zeroes sums_dev [3] (fp64, the epoch's loss sums that
 * bgx_ppo_rows adds to); grads adds (m0, m1, m2, m0 + c_value m1 - c_entropy m2), m = sums /
 * n_total, to parts_dev [4] in fp64 (the torch form's arithmetic, no contraction). */
int bgx_ppo_epoch_prep(const float* w1_dev, const float* b1_dev, const float* wa_dev, const float* ba_dev,
                       const float* wv_dev, const float* bv_dev, int32_t hidden, int32_t n_actions, void* w1pack_dev,
                       void* b1h_dev, void* w2h_dev, void* b2h_dev, float* gw1_dev, float* gw2_dev, float* gb2_dev,
                       float* hmax2_dev_or_null, float* bound_dev_or_null, double* sums_dev_or_null, void* stream);
int bgx_ppo_epoch_grads(const float* gw1_dev, const float* gw2_dev, const float* gb2_dev, int32_t hidden,
                        int32_t n_actions, float post, float* w1_grad, float* b1_grad, float* wa_grad, float* ba_grad,
                        float* wv_grad, float* bv_grad, const float* bound_dev, const float* hmax2_dev,
                        float limit, uint8_t* guard_dev_or_null, const double* sums_dev, double n_total,
                        double c_value, double c_entropy, double* parts_dev_or_null, void* stream);

/* The episode accounting of a [T][B] rollout (the reference driver's per-env loop,
 * train.py:55-99; bgx.train.episode_stats): records_dev uint8[T][B][64] (the mover is
 * byte 52), carry_dev fp64[B] = each lane's reward of its unfinished episode, updated in
 * place; out_dev fp64[6] = finished episodes, their summed rewards, wins, PLAYER1 wins,
 * gammon wins, backgammon wins.  workspace of bgx_episode_stats_workspace(B) bytes. */
int64_t bgx_episode_stats_workspace(int32_t B);
int bgx_episode_stats(const float* rewards_dev, const uint8_t* dones_dev, const uint8_t* records_dev,
                      double* carry_dev, int32_t T, int32_t B, double* workspace_dev, double* out_dev, void* stream);

/* The PPO update's rollout rows in a given order, once per update (the fused head's
 * row plan, bgx.train.ppo_row_plan; the reference batches memory rows in order,
 * ppo_agent.py:235-266): row i of each output = row perm[i] of its input, for the
 * 64-byte records and the four per-row fields (action, old log-prob, return,
 * advantage).  One kernel (16-byte copies of the records). */
/* csrc/bg_adam.hip.  The PPO optimizer step: torch.optim.Adam(fused=True) (ADAM_MODE::ORIGINAL; no weight
 * decay, amsgrad or maximize) as GradScaler.step + GradScaler.update drive it
 * (ppo_agent.py:302-305 `scaler.step(self.optimizer); scaler.update()`), for up to 8
 * fp32 tensors: params/grads/exp_avg/exp_avg_sq device pointers, steps = each tensor's
 * fp32 step counter (device scalar), numels element counts (host arrays of n).  With
 * scale (GradScaler._scale, fp32) non-null: a non-finite scaled gradient anywhere skips
 * the step (no parameter, moment or counter changes) and backs the scale off; else the
 * gradients are unscaled in place and the step is taken; growth_tracker (int32) and the
 * scale follow _amp_update_scale_.  scale = NULL: a plain Adam step.  found: an int32
 * device flag, zero before the first call (each call leaves it zero). */
int bgx_adam_step(int32_t n, float* const* params, float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, float* const* steps, const int64_t* numels, double lr, double beta1,
                  double beta2, double eps, float* scale, int32_t* growth_tracker, float growth_factor,
                  float backoff_factor, int32_t growth_interval, int32_t* found, void* stream);
/* The fused head's row plan for m rollout rows (replaces torch's argsort + bincount +
 * cumsum in bgx/train.py ppo_row_plan, which are its CPU / reference form): a row's class
 * is ceil(lim / 32) with lim = n_actions when its legal count (record bytes 60-61) is 0,
 * else min(count, n_actions); perm_dev int32[m] = the rows ordered by class, stably (the
 * order k_ppo_rows / k_ppo_gw2 read them in); plan_dev int32[33] = the k_ppo_gw2 task
 * prefix per action tile (17) then the first row tile reaching each action tile (16);
 * row_plan_dev int32[8] = the row-tile ranges of the bgx_ppo_rows variants.  Device
 * only, no host sync; workspace_dev: bgx_ppo_plan_workspace(m) bytes. */
int64_t bgx_ppo_plan_workspace(int32_t m);
int bgx_ppo_plan(const uint8_t* records_dev, int32_t m, int32_t n_actions, int32_t* workspace_dev, int32_t* perm_dev,
                 int32_t* plan_dev, int32_t* row_plan_dev, void* stream);
int bgx_gather_rollout(const int32_t* perm_dev, int32_t n, const uint8_t* records_dev, const int32_t* actions_dev,
                       const float* old_logp_dev, const float* returns_dev, const float* adv_dev,
                       uint8_t* records_out, int32_t* actions_out, float* old_logp_out, float* returns_out,
                       float* adv_out, void* stream);
/* bgx_ppo_plan and bgx_gather_rollout in one pass (round 6): the plan, and each row's
 * record and four fields written straight to its plan-order position (the scatter reads
 * the records once, coalesced; no perm pass, no random-read gather).  perm_or_null: the
 * permutation too (tests).  Same workspace; records and records_out 16-byte aligned. */
int bgx_ppo_plan_rows(const uint8_t* records_dev, int32_t m, int32_t n_actions, int32_t* workspace_dev,
                      const int32_t* actions_dev, const float* old_logp_dev, const float* returns_dev,
                      const float* adv_dev, uint8_t* records_out, int32_t* actions_out, float* old_logp_out,
                      float* returns_out, float* adv_out, int32_t* perm_or_null, int32_t* plan_dev,
                      int32_t* row_plan_dev, void* stream);

/* Phase times of the last bgx_two_ply call on e (first round, HIP events on the
 * caller's stream): ms2[0] = reply enumeration (all tiers), ms2[1] = leaf
 * evaluation after it (k_eval, the MFMA kernel). */
int bgx_two_ply_timings(bgx_engine* e, float* ms2);

/* Debug options (tests and diagnostics only; the product path never reads the
 * environment).  Sets option `name` to `value` (NULL: unset) for the process.  Names:
 * BGX_2PLY_HEAVY "log:memo" (9:0 / 10:0: the doubles enumerator without the memo / with
 * a 1,024-slot table), BGX_2PLY_LDS_CAP "first[:mid]" (forced overflow tiers),
 * BGX_2PLY_POOL n (leaf-pool slots: retry rounds), BGX_2PLY_UNFACTORED (the 13-k-block
 * evaluator), BGX_2PLY_BARROW 0 (bar rows per job), BGX_2PLY_DUMP path (pool, row sides,
 * V per slot), BGX_2PLY_DEBUG (round sizes on stderr), BGX_POLICY_SKIP 0 (no tile skip),
 * BGX_POLICY_HEAVY n (the policy's heavy-row bound), BGX_POLICY_ROWBEST 0 | 1 | 2 (the
 * policy's noise guard: on the lane's best key / on the row's, gathered rows of main waves
 * drawing nothing / that per quarter tile, the default); read at engine creation: BGX_XCD 0,
 * BGX_ORDER 0 (lane-order dispatch), BGX_STAMPS, BGX_STEP_DEBUG, BGX_TIER1_CAP n and
 * BGX_MOVEGEN_CAP n (the unique-afterstate caps of the step's first overflow tier and of
 * bgx_movegen's main table, clamped to [1, the table's own cap]).  Every alternative is
 * exact: results are identical, only the schedule or the diagnostics change. */
int bgx_debug_option(const char* name, const char* value_or_null);

/* Last HIP error string of this thread (diagnostics). */
const char* bgx_last_error(void);

/* Build provenance: sha256 (hex) of the sources and compile flags this library
 * was built from (bgx._lib.source_hash); smoke() and the tests compare it with
 * the tree they run from. */
const char* bgx_build_id(void);

#ifdef __cplusplus
}
#endif
#endif /* BGX_H */
