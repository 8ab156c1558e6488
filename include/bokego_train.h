/*
 * bokego_train.h -- C ABI of the training kernels (libbktrain.so): the trunk of the reference's PolicyNet / ValueNet
 * (bokego/nnet.py:31-57, 73-113) with gradients, for bokego_amd/train.py, the move sampler of the REINFORCE
 * playouts (bokego_amd/reinforce.py), and the Go rules and the area score of the device-resident playouts
 * (bokego_amd/reinforce.py, bokego_amd/genvals.py).
 *
 * Conventions:
 *   - Stateless.  No entry point allocates device memory or keeps anything between calls: every buffer is a device
 *     pointer the caller owns (torch tensors in bokego_amd/train.py, so torch's caching allocator holds all memory),
 *     scratch included (bkt_conv_wgrad_workspace, bkt_bn_workspace).
 *   - Every kernel is enqueued on `stream` (a hipStream_t; NULL = the null stream) and the call returns without
 *     waiting.  Returns BKT_OK (0) or a negative bkt_status; BKT_ERR_HIP means a launch failed.
 *   - Tensors are contiguous fp32 NCHW on the 9x9 board, [B, C, 9, 9]; conv weights are torch's [Cout, Cin, k, k]
 *     with Cout = 128.  Supported convolutions: k = 5 (pad 2) and k = 3 (pad 1), any Cin >= 1; the network uses
 *     5x5 27->128 and 3x3 128->128.  1 <= B <= BKT_MAX_BATCH.
 *   - Arithmetic: fp32 in, fp32 accumulate (v_mfma_f32_16x16x4_f32).  Every result is deterministic: sums run in
 *     an order fixed by the shapes alone (no float atomics), so equal inputs give equal bits.
 *   - The bkt_*_bf16 entry points are an opt-in mixed-precision form of the six convolution calls: the same fp32
 *     tensors, bf16 GEMM operands, fp32 accumulate (v_mfma_f32_16x16x32_bf16); see "bf16 mixed precision" below.
 *   - Non-finite values.  The convolutions and the BatchNorm + ReLU calls pass a NaN or an Inf on; none of them turns
 *     one into a finite number.  With ref the same operation in float64 (torch: conv2d and its two gradients,
 *     batch_norm + relu with autograd), for every element of every output:
 *       - got is finite exactly where ref is finite;
 *       - where ref is NaN, got is NaN;
 *       - where ref is +-Inf, got is the same Inf.  The fp32 convolutions may give NaN instead: their compensated
 *         sums compute (t - acc) - y, which is inf - inf once a running sum is Inf.  The bf16 convolutions (plain
 *         sums) and the BatchNorm calls give the Inf;
 *       - where ref is finite and does not depend on the non-finite input, got has the bits of the same call on
 *         finite inputs: no kernel's summation order depends on values, and a masked load mixes nothing in.
 *     In particular relu(NaN) is NaN and relu's gradient passes at a NaN output (the mask is "not y <= 0", torch's),
 *     a channel of bkt_bn_relu_train with one NaN or Inf in x is NaN in all its B*81 outputs, in save_invstd and in
 *     running_var (the variance is inf - inf; its clamp at 0 is for rounding only), and its save_mean and
 *     running_mean are the NaN or the Inf.  In the forward convolution zero padding is a multiplication by zero: a non-finite
 *     weight makes every point of its output channel non-finite, and Inf * 0 is NaN.  The input gradient has no padding to multiply: a
 *     non-finite weight reaches the points of its channel of dx whose tap lies on the board and no others (the
 *     GEMM takes such a weight as 0 and a second kernel adds its terms).  An infinite gamma is evaluated in
 *     torch's form x * a + (beta - mean * a), a = invstd * gamma, which is NaN where x and the mean have one sign.
 *     tests/nonfinite_cases.py has the cases; what reads the weights for inference refuses non-finite ones instead
 *     (include/bokego_amd.h, bk_engine_create).
 */
#ifndef BOKEGO_TRAIN_H
#define BOKEGO_TRAIN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BKT_ABI_VERSION 4
#define BKT_MAX_BATCH 65536
#define BKT_COUT 128
#define BKT_MAX_SAMPLE_ROWS (1 << 24)

typedef enum bkt_status {
    BKT_OK = 0,
    BKT_ERR_ARG = -1, /* null pointer, unsupported shape, workspace too small */
    BKT_ERR_HIP = -2  /* a kernel launch failed                              */
} bkt_status;

int bkt_abi_version(void);

/* ---- convolution (implicit GEMM: M = 128 output channels, N = B*81 points, K = Cin*k*k) ------------------------ */

/* w [128, cin, k, k] -> wt [cin*k*k, 128] (K-major), the operand layout of bkt_conv_forward. */
int bkt_conv_pack(const float *w, int cin, int ksize, float *wt, void *stream);

/* y = conv(x, w) + bias (bias may be NULL).  x [B, cin, 9, 9], wt from bkt_conv_pack, y [B, 128, 9, 9].
 * Taps that fall off the board read zero. */
int bkt_conv_forward(const float *x, const float *wt, const float *bias, float *y, int batch, int cin, int ksize,
                     void *stream);

/* 3x3 128->128 only: w [128, 128, 3, 3] -> wt_dgrad [128*9, 128], the filters rotated by 180 degrees with input and
 * output channels swapped, packed as bkt_conv_pack packs. */
int bkt_conv_pack_dgrad(const float *w, float *wt_dgrad, void *stream);

/* dx = dL/dx of the 3x3 128->128 convolution: the forward problem on dy with the bkt_conv_pack_dgrad filters.
 * dy, dx [B, 128, 9, 9].  Two launches: the second adds the terms of weights that are not finite ("Non-finite values")
 * and returns at once when there are none. */
int bkt_conv_dgrad(const float *dy, const float *wt_dgrad, float *dx, int batch, void *stream);

/* The batch is reduced in fixed slices of BKT_WGRAD_CHUNK boards: one partial result per slice, then the slices are
 * added in slice order. */
#define BKT_WGRAD_CHUNK 16

/* Bytes of scratch bkt_conv_wgrad needs: a [128, cin*k*k] fp32 partial and 128 x 2 double partials per slice
 * (0 for unsupported arguments). */
size_t bkt_conv_wgrad_workspace(int batch, int cin, int ksize);

/* dw [128, cin, k, k] = dL/dw and db [128] = dL/dbias (db may be NULL), from the layer input x [B, cin, 9, 9] and
 * dy = dL/dy [B, 128, 9, 9].  The batch is split into fixed chunks whose partial products go to `workspace`; a
 * second kernel sums the chunks in chunk order.  Overwrites dw and db (no accumulation into them). */
int bkt_conv_wgrad(const float *x, const float *dy, float *dw, float *db, int batch, int cin, int ksize,
                   void *workspace, size_t workspace_bytes, void *stream);

/* ---- bf16 mixed precision: the convolutions with bf16 operands (bk_train_bf16.hip) ---------------------------------- */

/* The six calls above, argument for argument, except that packed weights are uint16_t (bf16 bit patterns).
 *   - All tensors in memory stay fp32 with the shapes above: x, dy, w, bias, y, dx, dw, db.  Only the packed weights
 *     are bf16.
 *   - Each GEMM operand element is rounded ONCE to bf16, round to nearest even (a NaN stays a NaN), on its way into the
 *     matrix unit -- the weights in the pack call.  With r() that rounding: products are exact in fp32, sums are the
 *     MFMA's fp32 accumulation, without Kahan compensation.
 *       forward          y  = sum r(w) r(x) + bias          bias added in fp32, unrounded
 *       input gradient   dx = sum r(w rotated) r(dy)
 *       weight gradient  dw = sum r(dy) r(x)                per slice of BKT_WGRAD_CHUNK boards, slices added in order
 *       bias gradient    db = sum dy                        the UNROUNDED dy: double partials per slice, slices in order
 *   - Deterministic as the fp32 calls: no float atomics, sums in an order fixed by the shapes.
 *   - The same shapes: k = 5 or 3, any cin >= 1 (K is padded with zeros inside the packed operand), the input gradient
 *     for 3x3 128->128 only, 1 <= B <= BKT_MAX_BATCH.  Anything else: BKT_ERR_ARG.
 * The packed layout is private to the library: allocate bkt_conv_packed_elems_bf16 elements and pass them through. */

/* Number of uint16_t a packed operand of a [128, cin, k, k] weight holds, padding included (0 for unsupported
 * arguments).  bkt_conv_pack_dgrad_bf16 writes bkt_conv_packed_elems_bf16(128, 3): for that shape the count includes
 * a second half, in which the input gradient keeps the weights that are not finite. */
size_t bkt_conv_packed_elems_bf16(int cin, int ksize);

int bkt_conv_pack_bf16(const float *w, int cin, int ksize, uint16_t *wt, void *stream);

int bkt_conv_forward_bf16(const float *x, const uint16_t *wt, const float *bias, float *y, int batch, int cin,
                          int ksize, void *stream);

int bkt_conv_pack_dgrad_bf16(const float *w, uint16_t *wt_dgrad, void *stream);

int bkt_conv_dgrad_bf16(const float *dy, const uint16_t *wt_dgrad, float *dx, int batch, void *stream);

/* Bytes of scratch bkt_conv_wgrad_bf16 needs (the same amount as bkt_conv_wgrad_workspace). */
size_t bkt_conv_wgrad_workspace_bf16(int batch, int cin, int ksize);

int bkt_conv_wgrad_bf16(const float *x, const float *dy, float *dw, float *db, int batch, int cin, int ksize,
                        void *workspace, size_t workspace_bytes, void *stream);

/* ---- BatchNorm2d + ReLU over `channels` channels of B*81 values each ------------------------------------------------ */

/* Bytes of scratch bkt_bn_relu_train / bkt_bn_relu_backward need: channels x 2 doubles per slice of boards. */
size_t bkt_bn_workspace(int batch, int channels);

/* Train mode: batch mean and biased variance (per-slice sums of x and x^2 in double),
 * y = relu((x - mean) * invstd * gamma + beta), invstd = 1/sqrt(var + eps).
 * save_mean / save_invstd [channels] keep what bkt_bn_relu_backward needs.  When running_mean / running_var are
 * not NULL they are updated as torch does: r = (1 - momentum) * r + momentum * s, with the UNBIASED variance
 * var * n / (n - 1) (n = B*81) going into running_var; num_batches_tracked (int64, may be NULL) is incremented. */
int bkt_bn_relu_train(const float *x, const float *gamma, const float *beta, float *running_mean, float *running_var,
                      int64_t *num_batches_tracked, float momentum, float eps, float *y, float *save_mean,
                      float *save_invstd, void *workspace, size_t workspace_bytes, int batch, int channels,
                      void *stream);

/* Gradients of bkt_bn_relu_train: dy = dL/dy, y its output (the ReLU mask is y > 0, and open at a NaN y), x its input.
 * Writes dx [B, channels, 9, 9], dgamma and dbeta [channels]. */
int bkt_bn_relu_backward(const float *dy, const float *y, const float *x, const float *gamma, const float *save_mean,
                         const float *save_invstd, float *dx, float *dgamma, float *dbeta, void *workspace,
                         size_t workspace_bytes, int batch, int channels, void *stream);

/* Eval mode: y = relu((x - running_mean) / sqrt(running_var + eps) * gamma + beta). */
int bkt_bn_relu_eval(const float *x, const float *gamma, const float *beta, const float *running_mean,
                     const float *running_var, float eps, float *y, int batch, int channels, void *stream);

/* Gradients of bkt_bn_relu_eval (frozen statistics): m = [y > 0] (1 at a NaN y), invstd = 1/sqrt(running_var + eps),
 * dx = dy * m * gamma * invstd, dbeta = sum dy * m, dgamma = sum dy * m * (x - running_mean) * invstd.
 * y is bkt_bn_relu_eval's output, x its input.  The sums use per-slice double partials added in slice order, as
 * bkt_bn_relu_backward does, in a bkt_bn_workspace(batch, channels) scratch.  Writes dx [B, channels, 9, 9],
 * dgamma and dbeta [channels]. */
int bkt_bn_relu_eval_backward(const float *dy, const float *y, const float *x, const float *gamma,
                              const float *running_mean, const float *running_var, float eps, float *dx, float *dgamma,
                              float *dbeta, void *workspace, size_t workspace_bytes, int batch, int channels,
                              void *stream);

/* ---- move sampling (bokego_amd/reinforce.py) ------------------------------------------------------------------------ */

/* One wave64 per row b of logits [B, 81]: p_i = exp(x_i - max x), S = sum p (the inclusive prefix at i = 80).
 * A Philox4x32-10 draw with key (seed low word, seed high word) and counter counters[b] = (c0, c1, c2, c3) gives
 * u = (x0 >> 8) * 2^-24 in [0, 1); the move is the first i whose inclusive prefix of p exceeds u * S.  Legality is plane
 * 5 of the uint8 feature planes [B, 27, 9, 9] (nnet.features' "legal" plane): a sample that is not legal is replaced by
 * the legal point of the largest logit (lowest index on ties), and a row with no legal point gets -1.
 * moves [B] (int32) and logp [B] = log softmax(x) at the move (0 where the move is -1).
 * Degenerate rows.  A row is degenerate when any of its 81 logits is NaN or +inf, or when all 81 are -inf; a row of
 * finite and -inf logits with at least one finite is an ordinary row (a -inf point has p = 0 and is never drawn; when
 * every legal logit is -inf the draw lands outside the set and the replacement gives the lowest legal index).  On a
 * degenerate row no draw is made: the move is the replacement rule's -- the legal point of the largest logit, with NaN
 * ordered as -inf and the lowest index on ties, or -1 with no legal point -- whatever the counter, and logp[b] is NaN
 * (also where the move is -1), which is how the caller sees that the policy's logits were not finite.  On every row, of
 * either kind, moves[b] is -1 or a point of the set in 0..80, and no logit outside the row's 81 is read.
 * 1 <= B <= BKT_MAX_SAMPLE_ROWS (rows are independent: no trunk batch limit applies). */
int bkt_sample_moves(const float *logits, const uint8_t *planes, int batch, uint64_t seed, const uint32_t *counters,
                     int32_t *moves, float *logp, void *stream);

/* bkt_sample_moves with the acceptable set read from mask[b * mask_stride + i] != 0 (i < 81) instead of plane 5: the same
 * softmax, the same draw, the same replacement of a sample outside the set, -1 when the set is empty (a playout passes).
 * bkt_sample_moves(logits, planes, ...) IS bkt_sample_moves_masked(logits, planes + 5 * 81, 27 * 81, ...): one kernel. */
int bkt_sample_moves_masked(const float *logits, const uint8_t *mask, size_t mask_stride, int batch, uint64_t seed,
                            const uint32_t *counters, int32_t *moves, float *logp, void *stream);

/* ---- the Go rules on the device (reinforce.py, genvals.py; bk_playout.hip) --------------------------------------------- */

/* For each row b < batch: if moves[b] >= 0, play it on the 192-byte record pos[b] (bk_pos, include/bokego_go.h) and
 * refresh its liberty cache, in place; status[b] = 0 or the BK_ILLEGAL_* code (record untouched).  moves[b] < 0: the
 * record is untouched, status[b] = 0.  If planes != NULL, planes[b] = the 27 u8 planes of the record as it stands after
 * the call (the ones bk_features_batch_u8 computes from it).  1 <= batch <= BKT_MAX_BATCH.  Stateless, enqueued on
 * `stream`, as every bkt_* call.
 * Byte identity with the host: every record afterwards equals what bk_pos_play(p, m) followed by
 * bk_pos_liberties(p, tmp) leaves, all 192 bytes (board, libs, libs_valid, ko, last move, turn, hash, reserved). */
int bkt_play_moves(void *pos, const int32_t *moves, int batch, int32_t *status, uint8_t *planes, void *stream);

/* One ply of a playout that runs to the end of the game (bokego_amd/rollout.py).  Per row b < batch:
 *   over != NULL && over[b] != 0      the record is untouched, status[b] = 0 (the game has ended);
 *   moves[b] >= 0                     exactly bkt_play_moves;
 *   moves[b] == BK_PASS (-1)          the record becomes what bk_pos_play(p, BK_PASS) + bk_pos_liberties(p, tmp) leaves, all
 *                                     192 bytes; if its last move was already BK_PASS and over != NULL, over[b] = 1;
 *   moves[b] <= BKT_MOVE_NONE         the record is untouched, status[b] = 0.
 * planes (may be NULL): as bkt_play_moves.  playable (may be NULL) [batch, 81]: for the record as it stands after the call,
 * 1 where the side to move may play in a playout: bk_pos_is_legal(p, s) && bk_pos_possible_eye(p, s) != the mover's colour
 * (black on an even turn) -- it never fills its own one-point eye, by the reference's definition of one.
 * 1 <= batch <= BKT_MAX_BATCH, else BKT_ERR_ARG. */
#define BKT_MOVE_NONE (-2)
int bkt_playout_step(void *pos, const int32_t *moves, int batch, uint8_t *over, int32_t *status, uint8_t *planes,
                     uint8_t *playable, void *stream);

/* For each row b < batch: score[b] = bk_pos_area_score(&pos[b], komi) -- Tromp-Taylor area: stones, plus empty regions
 * bordered by one colour only; black - (white + komi), computed as (float)black - ((float)white + komi).
 * owner != NULL: owner[b*81 + s] = +1 black stone or black-only region, -1 white, 0 otherwise.
 * The records are read only.  1 <= batch <= BKT_MAX_BATCH; komi must be finite; else BKT_ERR_ARG. */
int bkt_area_score(const void *pos, int batch, float komi, float *score, int8_t *owner, void *stream);

/* Whole uniformly random playouts in ONE launch (bokego_amd/rollout.py random_playouts, playout_value): every
 * row b < batch plays on, in place, until two passes in a row end its game or max_plies moves have been played here.
 * Ply k = 0, 1, ... of a row that is not over:
 *   P = the playable set of the record as it stands (bkt_playout_step's `playable`: bk_pos_is_legal and not the mover's
 *       own eye by bk_pos_possible_eye), n = |P|;
 *   x0 = the first word of Philox4x32-10 with key (seed low word, seed high word) and counter (c0, c1 + k, c2, c3), where
 *       (c0, c1, c2, c3) = counters[b] and c1 + k wraps at 2^32;
 *   the move is BK_PASS when n == 0, else the (((x0 >> 8) * n) >> 24)-th point of P in ascending point order (integer
 *       arithmetic, uniform up to n * 2^-24; no float, no fallback rule);
 *   it is played exactly as bkt_playout_step plays it, all 192 bytes; a pass after a pass sets over[b] = 1.
 * A record whose last move is BK_PASS on entry ends with its first pass.  A row whose over[b] != 0 on entry is untouched
 * and gets plies[b] = 0.
 * plies[b] = the moves played here, passes included.  moves (may be NULL) [batch, max_plies] int16: the move of each ply,
 * BKT_MOVE_NONE from the ply at which the row was over (every entry is written).  status[b] = the bitwise or of the
 * BK_ILLEGAL_* codes of the row's plies (0: the playable set and the rules agree).  No feature planes are written; score
 * the final records with bkt_area_score.
 * 1 <= batch <= BKT_MAX_BATCH and 1 <= max_plies <= BKT_MAX_PLAYOUT_PLIES; pos, counters, over, plies and status must not
 * be NULL; else BKT_ERR_ARG and nothing is launched. */
#define BKT_MAX_PLAYOUT_PLIES 1024
int bkt_random_playouts(void *pos, int batch, uint64_t seed, const uint32_t *counters, int max_plies, uint8_t *over,
                        int32_t *plies, int16_t *moves, int32_t *status, void *stream);

/* The 3x3 pattern index of every point of every record (bokego_amd/patterns.py), occupied or not:
 * codes[b*81 + s] for s = 9r + c, relative to the record's side to move (black on an even turn).  The eight neighbours in
 * the order (dr, dc) = (-1,0) (+1,0) (0,-1) (0,+1) (-1,-1) (-1,+1) (+1,-1) (+1,+1) give a 2-bit state each -- 0 empty, 1 a
 * stone of the side to move, 2 an opponent stone, 3 off the board -- and code = sum of state_i << 2i (16 bits).  near = 1
 * when the record's last_move is a board point with max(|r - r_lm|, |c - c_lm|) <= 1, else 0 (a pass, no move).
 * index = near << 16 | code, in [0, BKT_PATTERN_ENTRIES).  The records are read only.
 * 1 <= batch <= BKT_MAX_BATCH; pos and codes must not be NULL; else BKT_ERR_ARG. */
#define BKT_PATTERN_ENTRIES 131072
int bkt_pattern_codes(const void *pos, int batch, int32_t *codes, void *stream);

/* Whole pattern-weighted playouts in ONE launch: bkt_random_playouts' contract in every respect except the draw.  table:
 * uint16 [BKT_PATTERN_ENTRIES] on the device; the weight of a point s is w_s = max(table[index of s], 1).  At a ply with
 * the playable set P and the same Philox word x0:
 *   S = the sum of w_s over P (at most 81 * 65535 < 2^23);  t = ((uint64_t)(x0 >> 8) * S) >> 24;
 *   the move is the first point of P, in ascending order, whose inclusive prefix sum of w exceeds t; BK_PASS when P is
 *   empty.  Integer arithmetic only: no float, no fallback rule.  A table of one constant plays bkt_random_playouts' games.
 * The argument checks are bkt_random_playouts'; a NULL table is BKT_ERR_ARG too, and nothing is launched. */
int bkt_pattern_playouts(void *pos, int batch, uint64_t seed, const uint32_t *counters, const uint16_t *table, int max_plies,
                         uint8_t *over, int32_t *plies, int16_t *moves, int32_t *status, void *stream);

/* The tactical code of every point of every record (bokego_amd/tactics.py), occupied or not:
 * codes[b*81 + q].  With F the 27 planes bk_features_batch_u8(record, fresh = 0) gives (a non-zero entry of planes 6..26
 * holds the count, capped at 7):
 *   cap = the value on planes 20..26 at q (stones captured by playing q), or 0;  C = min(cap, 3);
 *   la  = the value on planes 13..19 at q (liberties after playing q), or 0 when q is not legal;
 *         A = 0 for la <= 1, 1 for la == 2, 2 for la >= 3;
 *   E = 1 when some on-board 4-neighbour t of q has F[0][t] != 0 and F[6][t] != 0 (a stone of the side to move whose
 *       cached liberty count is 1);
 *   G = 1 when some on-board 4-neighbour t has F[1][t] != 0 and F[7][t] != 0 (an opponent stone whose cached count is 2);
 *   code = C | A << 2 | E << 4 | G << 5, in [0, BKT_TACTIC_ENTRIES).
 * The liberty planes are the reference's cache and can be stale: the code is a function of the record's bytes.
 * The records are read only.  1 <= batch <= BKT_MAX_BATCH; pos and codes must not be NULL; else BKT_ERR_ARG. */
#define BKT_TACTIC_ENTRIES 64
int bkt_tactical_codes(const void *pos, int batch, int32_t *codes, void *stream);

/* Whole tactical playouts in ONE launch: bkt_pattern_playouts' contract with a second table.  tactics: uint16
 * [BKT_TACTIC_ENTRIES] on the device, 256 = neutral; table: as bkt_pattern_playouts', or NULL for no patterns.  The weight
 * of a playable point s is
 *   P = max(table[pattern index of s], 1), or 256 when table is NULL;  T = tactics[tactical code of s];
 *   w_s = max(1, (P * T) >> 8)      (a 32-bit product; w_s < 2^24, so a row's sum S <= 81 * 2^24 < 2^31)
 * and the draw is bkt_pattern_playouts': t = ((uint64_t)(x0 >> 8) * S) >> 24 on the same Philox word, the first point of
 * P in ascending order whose inclusive prefix sum of w exceeds t, BK_PASS when P is empty.  A tactics table of 256
 * everywhere plays bkt_pattern_playouts' games, and with table NULL bkt_random_playouts' games, byte for byte.
 * The argument checks are bkt_pattern_playouts' except that table may be NULL; a NULL tactics is BKT_ERR_ARG. */
int bkt_tactical_playouts(void *pos, int batch, uint64_t seed, const uint32_t *counters, const uint16_t *table,
                          const uint16_t *tactics, int max_plies, uint8_t *over, int32_t *plies, int16_t *moves,
                          int32_t *status, void *stream);

/* The all-moves-as-first (AMAF) counts of whole playouts (bokego_amd/rollout.py playout_amaf), read from the
 * history the three bkt_*_playouts calls write.  moves [records * playouts, max_plies] int16: a point 0..80, BK_PASS, or
 * BKT_MOVE_NONE from the ply at which the row was over; rows r * playouts .. (r + 1) * playouts - 1 belong to record r.
 * won[row] != 0: the side to move at the record won that playout.  Ply 0 is that side's, so it plays the even plies.
 * For a row and a point s let k be the smallest ply with moves[row, k] == s, looking no further than the first entry
 * <= BKT_MOVE_NONE, which ends the row.  If k exists and is even, the row counts for s:
 *   played[r * 81 + s] += 1,  won_at[r * 81 + s] += (won[row] != 0).
 * A point the opponent played first does not count for the row, whatever is played there later; passes are skipped; an
 * entry above 80 is ignored (entries are compared, never used as an index).  Every entry of played and won_at
 * [records, 81] is written, zeros included.  Integers only: the counts do not depend on any order.
 * moves, won, played and won_at must not be NULL; records >= 1, playouts >= 1, records * playouts <= BKT_MAX_SAMPLE_ROWS,
 * 1 <= max_plies <= BKT_MAX_PLAYOUT_PLIES; else BKT_ERR_ARG and nothing is launched. */
int bkt_amaf_counts(const int16_t *moves, int max_plies, const uint8_t *won, int records, int playouts, int32_t *played,
                    int32_t *won_at, void *stream);

/* The same counts for both sides of every history: the AMAF records of the tree's RAVE tables (bk_pool_deliver_rave,
 * include/bokego_tree.h).  moves, won and the row-to-record mapping are bkt_amaf_counts'.  For a row and a point
 * s let k be the smallest ply with moves[row, k] == s, looking no further than the first entry <= BKT_MOVE_NONE.  If k
 * exists, the row counts for side k & 1 -- side 0 is the side to move at the record, side 1 its opponent, who wins the
 * rows with won[row] == 0:
 *   played[(r * 2 + (k & 1)) * 81 + s] += 1,
 *   won_at[(r * 2 + (k & 1)) * 81 + s] += ((won[row] != 0) == ((k & 1) == 0)).
 * A point counts once per row, for the side that played it first, so played[r, 0, s] + played[r, 1, s] <= playouts.
 * Passes are skipped; an entry above 80 is ignored (entries are compared, never used as an index).  Every entry of
 * played and won_at [records, 2, 81] is written, zeros included.  Integers only: the counts do not depend on any order,
 * and side 0 equals bkt_amaf_counts' output on the same input, integer for integer.
 * The argument checks are bkt_amaf_counts': else BKT_ERR_ARG, nothing is launched and nothing written. */
int bkt_amaf_counts_sides(const int16_t *moves, int max_plies, const uint8_t *won, int records, int playouts,
                          int32_t *played, int32_t *won_at, void *stream);

/* What the final boards of whole playouts say beyond who won (bokego_amd/rollout.py playout_ownership): the
 * ownership, agreement and score-margin counts of every record's playouts, scored and reduced in one launch.
 * pos holds records * playouts final 192-byte records (bk_pos), read only; rows r * playouts .. (r + 1) * playouts - 1
 * belong to record r (the layout of the three bkt_*_playouts calls' callers).  Board bytes are 0, 1 (black), 2 (white).
 * Per row: own[s] is exactly the owner bkt_area_score defines -- +1 for a black stone or a black-only empty region, -1 for
 * white, 0 otherwise;  B = #(own == +1), W = #(own == -1);  bw = ((float)B - ((float)W + komi)) > 0, bkt_area_score's
 * expression, so the row wins here if and only if its score > 0 there;  d = B - W.
 * Per record r, from zero:
 *   black[r * 81 + s] += (own[s] == +1),   white[r * 81 + s] += (own[s] == -1),
 *   agree[r * 81 + s] += (own[s] == +1 && bw) || (own[s] == -1 && !bw)     the point ended up with the row's winner,
 *   hist[r * 163 + d + 81] += 1            the margin before komi, d in -81 .. 81,
 *   black_wins[r] += bw.
 * Every entry of black, white, agree [records, 81], hist [records, 163] and black_wins [records] is written, zeros
 * included.  Integers only: the counts do not depend on any order.
 * No pointer but stream may be NULL; records >= 1, playouts >= 1, records * playouts <= BKT_MAX_SAMPLE_ROWS; komi must be
 * finite; else BKT_ERR_ARG, nothing is launched and nothing written. */
int bkt_owner_counts(const void *pos, int records, int playouts, float komi, int32_t *black, int32_t *white,
                     int32_t *agree, int32_t *hist, int32_t *black_wins, void *stream);

/* The move weights of every record, in ONE launch (bokego_amd/rollout.py move_weights, the pattern term of amaf_prior;
 * DESIGN 22): weights[b*81 + s] is the weight bkt_tactical_playouts' draw gives point s at the first ply of a playout
 * started from record b as it stands, and 0 where s is not in that ply's playable set.
 *   Playable: plane 5 of the 27 planes bk_features_batch_u8(record, fresh = 0) gives is non-zero at s, and s is not the
 *       mover's own one-point eye by bk_pos_possible_eye: the set bkt_playout_step leaves behind for an untouched record.
 *   P = max(table[index], 1) with index exactly bkt_pattern_codes' index of s; P = 256 when table is NULL.
 *   T = tactics[code] with code exactly bkt_tactical_codes' code of s; T = 256 when tactics is NULL.
 *   w_s = max(1, (P * T) >> 8) on the playable set (a 32-bit product; w_s < 2^24), 0 off it.
 * table: uint16 [BKT_PATTERN_ENTRIES] and tactics: uint16 [BKT_TACTIC_ENTRIES] on the device; both may be NULL, which
 * gives 256 on the playable set.  Every entry of weights [batch, 81] is written.  The records are read only.  Integers
 * only.
 * 1 <= batch <= BKT_MAX_BATCH; pos and weights must not be NULL; else BKT_ERR_ARG, nothing is launched and nothing
 * written. */
int bkt_move_weights(const void *pos, int batch, const uint16_t *table, const uint16_t *tactics, uint32_t *weights,
                     void *stream);

/* Last-good-reply playouts with forgetting (LGRF-1; bokego_amd/rollout.py ReplyTable): a reply table the
 * playouts of a search learn.  replies is uint8 [2][81], 162 bytes: replies[c][prev] is the reply of colour c (0 black,
 * 1 white) to the opponent's move on board point prev.  A value 0..80 is a point; BKT_REPLY_NONE = 255 means none; a value
 * above 80 other than 255 is treated as none.  A previous move that is a pass or "no move" has no entry.  Entries are
 * compared or bounds-checked before they index anything.
 *
 * Use (in a playout).  At a ply, take the side to move c, the last move lm and the playable set P that the ply body left
 * behind (legal, not an own one-point eye).  If lm is a board point, r = replies[c][lm] is a point and r is in P, the move
 * is r.  Otherwise the move is whatever the underlying draw picks: tactical, pattern, or uniform when both tables are NULL.
 * The Philox word of a ply is indexed by the ply, so skipping the draw shifts nothing.
 *
 * bkt_reply_playouts is bkt_tactical_playouts' contract with `replies` put in, read only, on the device.  table and tactics
 * may each be NULL, and both may be NULL; replies == NULL returns BKT_ERR_ARG and nothing is launched.  With every entry
 * 255 the records, histories, plies, over and status are byte for byte those of bkt_tactical_playouts (both tables, or
 * tactics alone), bkt_pattern_playouts (table alone) or bkt_random_playouts (neither). */
#define BKT_REPLY_NONE 255
int bkt_reply_playouts(void *pos, int batch, uint64_t seed, const uint32_t *counters, const uint16_t *table,
                       const uint16_t *tactics, const uint8_t *replies, int max_plies, uint8_t *over, int32_t *plies,
                       int16_t *moves, int32_t *status, void *stream);

/* Update (after a batch of playouts).  pos [records, 192]: the starting records, read only; the side to move and the last
 * move of ply 0 come from them.  moves [records * playouts, max_plies] and won[row], exactly as bkt_amaf_counts_sides takes
 * them.  The result is defined as a sequential fold: rows ascending, plies ascending within a row, up to the first entry
 * <= BKT_MOVE_NONE or max_plies.  For ply t of a row:
 *   the mover's colour is c = (colour to move at the record) xor (t & 1);
 *   prev is the record's last move for t = 0, else moves[row, t - 1];   m = moves[row, t];
 *   if m or prev is not a board point, nothing happens;
 *   if the mover won the row, (won[row] != 0) == (t even), then replies[c][prev] = m;
 *   otherwise, if replies[c][prev] == m, then replies[c][prev] = 255.
 * The table is updated in place.  Entries with no event keep their value, whatever it is.
 * Two launches on `stream`, nothing waits on the host: the first, one workgroup per record, writes for every table entry a
 * summary of what the record's rows do to it (the points forgotten before the first store, and the value after the last
 * one) to scratch; the second composes the records' summaries in order and applies them to replies.  Integers only, no
 * atomics, no workgroup waits on another: the result is the fold's for every input, whatever the scheduling.
 * scratch: bkt_reply_scratch_bytes(records) = records * 2592 bytes on the device, 4-byte aligned; its contents on entry do
 * not matter, and all of it is written.
 * No pointer but stream may be NULL; records >= 1, playouts >= 1, records * playouts <= BKT_MAX_SAMPLE_ROWS,
 * 1 <= max_plies <= BKT_MAX_PLAYOUT_PLIES; else BKT_ERR_ARG, nothing is launched and nothing written. */
size_t bkt_reply_scratch_bytes(int records);
int bkt_reply_update(const void *pos, const int16_t *moves, int max_plies, const uint8_t *won, int records, int playouts,
                     uint8_t *replies, void *scratch, void *stream);

/* Many tables at once (a table per game of a self-play batch).  The use rule and the update rule are the two
 * above; new is only which table a row uses.  replies is uint8 [tables][2][81] on the device, and slots, int32 on the
 * device, names a table per row: slots[i] is the table of row i of bkt_reply_playouts_tables (batch entries) and of record
 * i of bkt_reply_update_tables (records entries).  A slot outside 0..tables-1 is compared before it indexes anything: such
 * a row plays as if its table were all 255, and such a record updates no table.  1 <= tables <= BKT_MAX_BATCH.
 * bkt_reply_playouts_tables: one launch; with tables = 1 and every slot 0 it is bkt_reply_playouts byte for byte.
 * bkt_reply_update_tables: table t becomes what bkt_reply_update makes of it with the records whose slot is t, in ascending
 * record order; a table that no record names keeps every byte, whatever it is.  Two launches: bkt_reply_update's first, and
 * one in which every table is owned by exactly one workgroup.  Integers only, no atomics, no workgroup waits on another.
 * scratch: bkt_reply_scratch_bytes(records), as above.
 * replies == NULL or slots == NULL returns BKT_ERR_ARG, nothing is launched and nothing is written; the other argument checks
 * are those of bkt_reply_playouts and bkt_reply_update. */
int bkt_reply_playouts_tables(void *pos, int batch, uint64_t seed, const uint32_t *counters, const uint16_t *table,
                              const uint16_t *tactics, const uint8_t *replies, int tables, const int32_t *slots,
                              int max_plies, uint8_t *over, int32_t *plies, int16_t *moves, int32_t *status, void *stream);
int bkt_reply_update_tables(const void *pos, const int16_t *moves, int max_plies, const uint8_t *won, int records,
                            int playouts, uint8_t *replies, int tables, const int32_t *slots, void *scratch, void *stream);

/* Replies keyed by the last two moves (LGRF-2, Baier & Drake 2010; bokego_amd/replies.py ReplyTable2).
 * replies2 is uint8 [2][82][81], 13284 bytes, 4-byte aligned (a misaligned pointer is BKT_ERR_ARG).
 * replies2[c][p2][p1] with p2 < 81 is the reply of colour c to the opponent's move on p1 that followed c's own move on p2.
 * Plane p2 == 81 is the LGRF-1 table: replies2[c][81][p1] is replies[c][p1] above.  Values are as there: 0..80 a point,
 * BKT_REPLY_NONE none, any other value above 80 treated as none and compared before it indexes anything.
 *
 * Use (in a playout).  c is the side to move, p1 the last move, p2 the move played two plies ago in this playout, P the
 * playable set.  At ply 1, p2 is the record's last move; at ply 0 there is no p2, because a record holds one move.
 *   if p1 and p2 are board points and replies2[c][p2][p1] is a point of P, that is the move;
 *   else, if p1 is a board point and replies2[c][81][p1] is a point of P, that is the move;
 *   else the inner draw decides (uniform, pattern or tactical, as in bkt_reply_playouts).
 * A pass or "no move" as p1 asks nothing; as p2 it skips the pair lookup only.  The Philox word stays indexed by the ply.
 *
 * bkt_reply2_playouts is bkt_reply_playouts' contract with replies2 in place of replies: one launch, one table for all
 * rows.  replies2 == NULL or misaligned returns BKT_ERR_ARG and nothing is launched.  With planes 0..80 all 255 it plays
 * bkt_reply_playouts' games with plane 81 as the table, byte for byte.
 *
 * Update.  The sequential fold of bkt_reply_update: rows ascending, plies ascending up to the first entry <= BKT_MOVE_NONE
 * or max_plies.  An event is a ply t whose move m and whose p1 are board points (p1: the record's last move at t = 0, else
 * moves[row, t - 1]); it is applied to entry [c][81][p1], and when p2 is a board point (the record's last move at t = 1,
 * moves[row, t - 2] from t = 2 on) also to entry [c][p2][p1]: a mover who won the row stores m; a mover who lost clears the
 * entry if it holds m.  Entries without an event keep their value, whatever it is.  Plane 81 therefore ends as
 * bkt_reply_update leaves replies from the same start.
 * bkt_reply2_update computes that fold event-parallel, in four launches on `stream`: the scratch is initialised; every
 * winner's event takes a 64-bit atomic max of (row * max_plies + t + 1) << 8 | m on its entries' keys; every loser's event
 * reads the key and the table and flags the entry when its m would clear it (a later clear of the last store's value, or
 * with no store a clear of the value on entry); one thread per entry writes the table.  Integers only; integer max is
 * order-independent and a flag is only ever written with one value, so the result is the fold's whatever the scheduling.
 * scratch: bkt_reply2_scratch_bytes() = 119556 bytes on the device, 8-byte aligned, whatever `records`; its contents on
 * entry do not matter.  The argument checks are bkt_reply_update's; else BKT_ERR_ARG, nothing launched, nothing written. */
int bkt_reply2_playouts(void *pos, int batch, uint64_t seed, const uint32_t *counters, const uint16_t *table,
                        const uint16_t *tactics, const uint8_t *replies2, int max_plies, uint8_t *over, int32_t *plies,
                        int16_t *moves, int32_t *status, void *stream);
size_t bkt_reply2_scratch_bytes(void);
int bkt_reply2_update(const void *pos, const int16_t *moves, int max_plies, const uint8_t *won, int records, int playouts,
                      uint8_t *replies2, void *scratch, void *stream);

/* Many pair tables at once (a pair table per game of a self-play batch).  The use rule and the update rule are
 * the two above; new is only which table a row uses.  replies2 is uint8 [tables][2][82][81] on the device, 4-byte aligned
 * (13284 is a multiple of 4, so every table is; a misaligned pointer is BKT_ERR_ARG), and slots, int32 on the device, has
 * the meaning it has for bkt_reply_playouts_tables: slots[i] is the table of row i of bkt_reply2_playouts_tables (batch
 * entries) and of record i of bkt_reply2_update_tables (records entries).  A slot outside 0..tables-1 is compared before
 * it indexes anything: such a row plays as if its table were all 255, and such a record updates no table.
 * 1 <= tables <= BKT_MAX_REPLY2_TABLES.
 * bkt_reply2_playouts_tables: one launch.  Plane 81 of a row's table is staged in LDS as bkt_reply_playouts_tables stages a
 * single table; the pair planes stay in global memory, and a thread reads its row's one pair byte per ply.  With tables = 1
 * and every slot 0 it is bkt_reply2_playouts byte for byte; with planes 0..80 of every table all 255 it is
 * bkt_reply_playouts_tables on the plane-81s byte for byte.
 * bkt_reply2_update_tables: table t becomes what bkt_reply2_update makes of it with the records whose slot is t, in
 * ascending record order; a table that no record names keeps every byte, whatever it is; plane 81 of every table ends as
 * bkt_reply_update_tables leaves it from the same start.  bkt_reply2_update's four launches with the entry index offset by
 * slot * 13284: integers only, and the result does not depend on the scheduling.
 * scratch: bkt_reply2_tables_scratch_bytes(tables) = tables * 119556 bytes on the device, 8-byte aligned (0 when tables is
 * outside 1..BKT_MAX_REPLY2_TABLES); its contents on entry do not matter.
 * replies2 == NULL or misaligned, slots == NULL, a misaligned scratch or tables out of range returns BKT_ERR_ARG; the other
 * argument checks are those of bkt_reply2_playouts and bkt_reply2_update.  A refused call launches nothing and writes
 * nothing. */
#define BKT_MAX_REPLY2_TABLES 4096
int bkt_reply2_playouts_tables(void *pos, int batch, uint64_t seed, const uint32_t *counters, const uint16_t *table,
                               const uint16_t *tactics, const uint8_t *replies2, int tables, const int32_t *slots,
                               int max_plies, uint8_t *over, int32_t *plies, int16_t *moves, int32_t *status, void *stream);
size_t bkt_reply2_tables_scratch_bytes(int tables);
int bkt_reply2_update_tables(const void *pos, const int16_t *moves, int max_plies, const uint8_t *won, int records,
                             int playouts, uint8_t *replies2, int tables, const int32_t *slots, void *scratch, void *stream);

/* One minorization-maximization (MM) pass over packed positions, in ONE launch: the sums a joint fit of the pattern and the
 * tactics table needs (bokego_amd/mmfit.py, whose sums_host is the definition in numpy).  The move model is the
 * playouts': a playable point j of a row has a pattern index i_j and a tactical code c_j and the strength gamma_p[i_j] *
 * gamma_t[c_j]; the move is drawn in proportion to it.
 *   codes  uint32 [rows, 81], one word per point: bits 0..16 bkt_pattern_codes' index, bits 17..22 bkt_tactical_codes'
 *          code, bit 31 set when the point is in the playable set, every other bit zero (bits 23..30 are ignored);
 *   moves  int32 [rows]: the move played from the row's position; below 0 (a pass, BKT_MOVE_NONE) or above 80: no point;
 *   gp     uint32 [BKT_PATTERN_ENTRIES], gt uint32 [BKT_TACTIC_ENTRIES]: the strengths in fixed point, gamma = g / 65536.
 *          Domain: 2^8 <= g <= 2^24 (gamma in [2^-8, 2^8]).  The caller guarantees it (the Python binding checks it); the
 *          kernel assumes it.  Outside it no access goes out of bounds, but the sums below may wrap.
 * Per row r, in unsigned 64-bit integers, over the playable points j of the row:
 *   s_j = max(1, (gp[i_j] * gt[c_j]) >> 16);   total[r] = E_r = the sum of s_j (0 for a row with no playable point).
 *   If moves[r] is a playable point m of the row: chosen[r] = s_m; rank[r] = the number of playable j with s_j > s_m, or
 *   with s_j == s_m and j < m; and for EVERY playable j
 *       den_p[i_j] += (gt[c_j] << 32) / E_r        den_t[c_j] += (gp[i_j] << 32) / E_r
 *   (floor division, each candidate on its own).  Otherwise -- a pass, no move, a move on a point that is not playable,
 *   such as an eye fill, a row with no playable point -- chosen[r] = 0, rank[r] = -1 and the row adds nothing; E_r = 0
 *   never reaches a division.
 * den_p uint64 [BKT_PATTERN_ENTRIES] and den_t uint64 [BKT_TACTIC_ENTRIES] are accumulated with +=: the caller zeroes them,
 * and several calls add up.  total, chosen (uint64 [rows]) and rank (int32 [rows]) are written for every row.  Integer
 * sums: the result does not depend on the scheduling, and the host mirror gives the same integers.
 * No wrap.  In the domain gp * gt >= 2^16, so s_j is the floor of x = gp * gt / 2^16 >= 1 and x < 2 s_j.  One row adds to
 * ALL of den_p, weighted by gp:  sum_j gp[i_j] * floor(gt[c_j] 2^32 / E_r) <= 2^48 * sum_j x_j / E_r < 2^49, so one row
 * adds less than 2^49 / gp[i] <= 2^41 to any one den_p[i], and likewise to any den_t[c].  A call of BKT_MM_MAX_ROWS = 2^14
 * rows stays below 2^55, and sums accumulated over fewer than 2^22 rows below 2^63.  Inside a row: s_j <= 2^32,
 * E_r <= 81 * 2^32 < 2^39, and a dividend is at most 2^24 << 32 = 2^56.
 * 1 <= rows <= BKT_MM_MAX_ROWS and no pointer but stream may be NULL; else BKT_ERR_ARG, nothing is launched and nothing
 * written. */
#define BKT_MM_MAX_ROWS 16384
#define BKT_MM_G_MIN (1u << 8)
#define BKT_MM_G_MAX (1u << 24)
int bkt_mm_sums(const uint32_t *codes, const int32_t *moves, int rows, const uint32_t *gp, const uint32_t *gt,
                uint64_t *den_p, uint64_t *den_t, uint64_t *total, uint64_t *chosen, int32_t *rank, void *stream);

/* The gradient sums of simulation balancing, in ONE launch: bkt_tactical_playouts whose draw also books, at every ply of
 * every playout, each candidate's share of the draw against its pattern index and its tactical code (bokego_amd/balance.py,
 * whose sums_host is the definition in numpy).  pos, batch, seed, counters, max_plies, over, plies, moves and
 * status are bkt_tactical_playouts'; table and tactics may each be NULL as in bkt_reply_playouts (a NULL pattern table is
 * 256 everywhere, a NULL tactics table likewise).  The games are untouched: records, over, plies, moves and status come
 * out byte for byte as bkt_tactical_playouts writes them for the same seed, counters and tables (with neither table, as
 * bkt_random_playouts writes them).
 *   coef    int32 [batch] on the device: one signed coefficient per row, |coef| <= BKT_BALANCE_MAX_COEF.  The caller
 *           guarantees the range (the Python binding checks it); outside it nothing goes out of bounds, but the sums may
 *           wrap.  A row whose coef is 0 books nothing.
 *   grad_p  int64 [BKT_PATTERN_ENTRIES], grad_t int64 [BKT_TACTIC_ENTRIES] on the device, 8-byte aligned: accumulated with
 *           +=; the caller zeroes them, and several calls add up.
 * With Q = BKT_BALANCE_Q: for every row b and every ply at which the row is not over and the total S of the draw's weights
 * is positive (a pass books nothing), with m the point the draw picks, every playable point j of weight w_j (the weight
 * bkt_move_weights defines), pattern index i_j (bkt_pattern_codes') and tactical code c_j (bkt_tactical_codes') books
 *       d_j = (j == m ? 2^Q : 0) - floor(w_j * 2^Q / S)
 *       grad_p[i_j] += coef[b] * d_j        grad_t[c_j] += coef[b] * d_j
 * d_j / 2^Q is the derivative of log(w_m / S) by the logarithm of either table entry of j, to within 2^-Q.  Integer sums
 * mod 2^64 (a signed accumulator through unsigned adds): the result does not depend on the scheduling, and the host mirror
 * gives the same integers.
 * No wrap.  Within one ply of one row the floors sum to at most 2^Q (they are the floors of shares that sum to 1) and the
 * picked point adds 2^Q once, so a ply changes any one entry by at most |coef| * 2^(Q+1) <= 2^12 * 2^25 = 2^37 in
 * magnitude; a row of at most BKT_MAX_PLAYOUT_PLIES = 2^10 plies by at most 2^47; a call of BKT_BALANCE_MAX_ROWS = 2^14 rows
 * by at most 2^61.  Sums over several calls belong in wider arithmetic than the accumulator (balance.py adds them up on the
 * host).  Inside a ply: w_j < 2^24, so w_j * 2^Q < 2^48, and S < 2^31.
 * 1 <= batch <= BKT_BALANCE_MAX_ROWS; coef, grad_p, grad_t and what bkt_tactical_playouts requires (but for the tables)
 * must not be NULL; else BKT_ERR_ARG, nothing is launched and nothing written. */
#define BKT_BALANCE_Q 24
#define BKT_BALANCE_MAX_ROWS 16384
#define BKT_BALANCE_MAX_COEF 4096
int bkt_balance_sums(void *pos, int batch, uint64_t seed, const uint32_t *counters, const uint16_t *table,
                     const uint16_t *tactics, const int32_t *coef, int64_t *grad_p, int64_t *grad_t, int max_plies,
                     uint8_t *over, int32_t *plies, int16_t *moves, int32_t *status, void *stream);

/* MAST playouts: per-move win rates the playouts of a search learn (the move-average sampling technique, Finnsson &
 * Bjornsson 2008; bokego_amd/movevalues.py MoveValueTable).  A move-value table has three parts, all integers:
 *   counts  int64 [2][81][2] on the device, 8-byte aligned: counts[c][m] = {played, won} of colour c (0 black = the mover
 *           on an even turn, 1 white) on point m, 0 <= won <= played;
 *   values  uint16 [2][81]: the factor of the draw's weight in units of 1/256, every entry >= 1, 256 = neutral;
 *   lut     uint16 [65], every entry >= 1, supplied by the caller: the value of a win rate i / 64.
 *
 * Use (in a playout).  bkt_move_value_playouts is bkt_tactical_playouts' contract in every respect, draw included, except
 * the weight.  table and tactics may each be NULL (a NULL tactics table is 256 everywhere, as in bkt_reply_playouts; both
 * NULL: w_in = 256).  With w_in the weight that draw gives a playable point q (bkt_move_weights defines it) and c the
 * colour to move at the ply,
 *   w = min(2^24 - 1, max(1, ((uint64_t)w_in * values[c][q]) >> 8))
 * so a row's sum S < 2^31 as before; the Philox word, t = ((x0 >> 8) * S) >> 24 and the prefix rule are the same.  With
 * values all 256 the records, over, plies, moves and status are bkt_tactical_playouts' byte for byte, and with table NULL
 * as well bkt_random_playouts'.  replies is NULL or bkt_reply_playouts' table, uint8 [2][81]; replies2 is NULL or
 * bkt_reply2_playouts' table, uint8 [2][82][81], 4-byte aligned; at most one of the two may be given.  A playable reply
 * overrules the draw exactly as in bkt_reply_playouts / bkt_reply2_playouts, and with values all 256 the games are those
 * entry points' games byte for byte.  One launch; values is read before the first ply and staged in LDS.
 * values == NULL, both reply tables given, a misaligned replies2, or any argument bkt_tactical_playouts refuses (but for the
 * tables) returns BKT_ERR_ARG; nothing is launched and nothing is written.
 *
 * Update (after a batch of playouts).  pos [records, 192], moves [records * playouts, max_plies] and won[row] are exactly
 * what bkt_reply_update takes: the starting records, and rows r * playouts .. (r + 1) * playouts - 1 belonging to record r.
 * For a row and every ply t before the first entry <= BKT_MOVE_NONE (or max_plies), with m = moves[row, t] in 0..80:
 *   c = (colour to move at record r) xor (t & 1);
 *   counts[c][m].played += 1;   counts[c][m].won += ((won[row] != 0) == (t even)).
 * Passes are skipped; an entry above 80 is ignored (entries are compared, never used as an index).  Every play counts:
 * there is no first-play rule, so a point retaken after a capture counts again.  After all rows are added, every entry:
 *   1. if limit > 0 and played >= limit, both fields are shifted right by the smallest s with played >> s < limit (old
 *      counts are forgotten, so the table follows the search as the game moves on);
 *   2. i = floor(64 * (2 * won + k) / (2 * (played + k))), in 0..64 because won <= played (k virtual plays at one half:
 *      an entry never played has i = 32);
 *   3. values[c][m] = lut[i].
 * Every entry of values is written.  The sums do not depend on any order, and the shift depends only on the sequence of
 * calls.  Two launches on `stream`, nothing waits on the host: the first, one workgroup per record, writes the record's
 * int32 partial counts to scratch by plain stores; the second sums them over the records, adds them into counts and applies
 * the shift and the lut.  Integers only, no atomics: the result is the definition's for every input, whatever the scheduling.
 * No wrap.  A record's partial counts are at most playouts * max_plies < 2^31.  A call adds at most records * playouts *
 * max_plies <= 2^24 * 2^10 = 2^34 to an entry.  With limit > 0 an entry is below limit <= 2^30 after every call, so it
 * never exceeds 2^30 + 2^34.  With limit == 0 the counts only grow, and the caller keeps played below 2^54 (more than 2^20
 * calls of the largest size): 64 * (2 * won + k) then stays below 2^62.
 * scratch: bkt_move_value_scratch_bytes(records) = records * 1296 bytes on the device, 4-byte aligned (0 when records < 1);
 * its contents on entry do not matter.
 * Domain: 1 <= k <= BKT_MOVE_VALUE_MAX_K; limit == 0 or 2 <= limit <= BKT_MOVE_VALUE_MAX_LIMIT; playouts * max_plies <
 * 2^31; no pointer but stream may be NULL; counts 8-byte aligned; otherwise bkt_reply_update's checks.  Else BKT_ERR_ARG:
 * a refused call launches nothing and writes nothing. */
#define BKT_MOVE_VALUE_NEUTRAL 256
#define BKT_MOVE_VALUE_MAX_K 65536
#define BKT_MOVE_VALUE_MAX_LIMIT (1 << 30)
int bkt_move_value_playouts(void *pos, int batch, uint64_t seed, const uint32_t *counters, const uint16_t *table,
                            const uint16_t *tactics, const uint16_t *values, const uint8_t *replies, const uint8_t *replies2,
                            int max_plies, uint8_t *over, int32_t *plies, int16_t *moves, int32_t *status, void *stream);
size_t bkt_move_value_scratch_bytes(int records);
int bkt_move_value_update(const void *pos, const int16_t *moves, int max_plies, const uint8_t *won, int records, int playouts,
                          int64_t *counts, uint16_t *values, const uint16_t *lut, int k, int limit, void *scratch,
                          void *stream);

/* A move-value table per game of a self-play batch (bokego_amd/movevalues.py MoveValueTables): the two calls
 * above over `tables` tables that share one lut, one k and one limit.
 *   counts  int64 [tables][2][81][2] on the device, 8-byte aligned;
 *   values  uint16 [tables][2][81];
 *   lut     uint16 [65], k, limit: as above, one for all tables;
 *   slots   int32 [batch] for the playouts, [records] for the update: the table of a row, or of a record.
 * 1 <= tables <= BKT_MAX_MOVE_VALUE_TABLES.  A slot outside 0..tables-1 is compared before it indexes anything: such a row
 * plays as if every value were 256, and such a record updates nothing.
 * bkt_move_value_playouts_tables: one launch.  Row i draws by the weight rule above with values[slots[i]]; the values of a
 * workgroup's three rows are staged in LDS before the first ply.  replies is NULL or uint8 [tables][162], a single reply
 * table per game under bkt_reply_playouts_tables' rule; replies2 is NULL or uint8 [tables][2][82][81], 4-byte aligned, a
 * pair table per game under bkt_reply2_playouts_tables' rule; at most one of replies and replies2 may be given.  The same
 * slots and the same tables name the reply table and the move-value table of a row.  With tables == 1 and every slot 0 it is
 * bkt_move_value_playouts byte for byte.  With every value 256 the games are those of bkt_tactical_playouts,
 * bkt_reply_playouts_tables and bkt_reply2_playouts_tables byte for byte, their uniform forms included (table and tactics
 * NULL).
 * bkt_move_value_update_tables: the update rule above applies per table, over the records whose slot names that table.  A
 * table that is named gets every entry of values written.  A table that no record names keeps every byte, even when its
 * played is at or above limit and even when its values are not what its counts imply.  A record with a slot outside the
 * range updates nothing.  Two launches on `stream`: the first is bkt_move_value_update's; the second, a workgroup per
 * (16 entries, table), adds the partial counts of the records that name its table.  Integers only, no atomics: the result is
 * the definition's, whatever the scheduling.  With tables == 1 and every slot 0 it is bkt_move_value_update byte for byte.
 * scratch: bkt_move_value_tables_scratch_bytes(records, tables) = records * 1296 bytes on the device, 4-byte aligned (0 when
 * records < 1 or tables is outside 1..BKT_MAX_MOVE_VALUE_TABLES); its contents on entry do not matter.
 * Domain checks: values == NULL, slots == NULL, tables out of range, both reply tables given or a misaligned replies2
 * returns BKT_ERR_ARG; the other checks are those of bkt_move_value_update and bkt_reply2_update_tables.  A refused call
 * launches nothing and writes nothing. */
#define BKT_MAX_MOVE_VALUE_TABLES 4096
int bkt_move_value_playouts_tables(void *pos, int batch, uint64_t seed, const uint32_t *counters, const uint16_t *table,
                                   const uint16_t *tactics, const uint16_t *values, const uint8_t *replies,
                                   const uint8_t *replies2, int tables, const int32_t *slots, int max_plies, uint8_t *over,
                                   int32_t *plies, int16_t *moves, int32_t *status, void *stream);
size_t bkt_move_value_tables_scratch_bytes(int records, int tables);
int bkt_move_value_update_tables(const void *pos, const int16_t *moves, int max_plies, const uint8_t *won, int records,
                                 int playouts, int64_t *counts, uint16_t *values, const uint16_t *lut, int k, int limit,
                                 int tables, const int32_t *slots, void *scratch, void *stream);

/* NAST playouts: move values keyed by the previous move (the N-gram average sampling technique, Powley, Whitehouse & Cowling
 * 2013; the N-gram selection of Tak, Winands & Bjornsson 2012; bokego_amd/movecontexts.py MoveContextTable).  A
 * move-context table is the move-value table above with a plane per previous move, all integers:
 *   counts  int64 [2][82][81][2] on the device, 8-byte aligned: counts[c][p][m] = {played, won} of colour c on point m played
 *           directly after move p (by either side); p == 81: after anything -- the move-value table above, as plane 81 of a
 *           pair reply table is the single one; 0 <= won <= played;
 *   values  uint16 [2][82][81]: the factor of the draw's weight in units of 1/256, every entry >= 1, 256 = neutral;
 *   lut     uint16 [65], k, limit: exactly the move-value table's;
 *   min_plays, 1 <= min_plays <= BKT_MOVE_CONTEXT_MAX_MIN_PLAYS: the plays a context entry needs before it counts.
 * The previous move.  In a playout it is the move played immediately before the ply, by either side, a pass included; at
 * ply 0 the record's last move.  In the update, p of ply t is moves[row, t - 1], and the record's last move for t == 0.
 * Anything outside 0..80 (a pass, none, junk) is p = 81; the value is compared before it indexes.
 *
 * Use.  bkt_move_context_playouts is bkt_move_value_playouts' contract in every respect -- the arguments, the NULL rules of
 * table and tactics, the rules of replies and replies2, every refused call -- except that values is the [2][82][81] table and
 *   w = min(2^24 - 1, max(1, ((uint64_t)w_in * values[c][p][q]) >> 8)).
 * One launch; nothing is staged: a thread reads exactly one uint16 of values per ply from global memory, and all fallback
 * logic lives in the update.  With values all 256 the games are those of bkt_tactical_playouts, bkt_random_playouts,
 * bkt_reply_playouts and bkt_reply2_playouts byte for byte; with every plane of a colour equal to its plane 81 they are
 * bkt_move_value_playouts' on that plane.
 *
 * Update.  bkt_move_context_update takes rows, won, the colour rule and the end-of-row rule exactly as bkt_move_value_update
 * does.  For every ply with a board point m:
 *   counts[c][81][m] += (1, mover won) always;   counts[c][p][m] += (1, mover won) when p < 81.
 * After all rows are added, every one of the 13,284 entries on its own is shifted right until played < limit (limit > 0);
 *   i1[c][m] = floor(64 * (2 * won + k) / (2 * (played + k))) of plane 81, and values[c][81][m] = lut[i1];
 *   for p < 81: values[c][p][m] = lut[(i1 + i2) >> 1] if the entry's played >= min_plays (after the shift), i2 the same
 *   index of the entry's own counts; else values[c][81][m].
 * Every entry of values is written.  Plane 81 of counts and values is byte for byte what bkt_move_value_update leaves on the
 * same inputs, and with min_plays >= limit > 0 no context ever qualifies.  Three launches on `stream`, nothing waits on the
 * host: the first zeroes scratch; the second, a wave per row, adds every play into scratch -- plane 81 summed per workgroup
 * in LDS first -- by 64-bit integer atomic adds; the third, a workgroup per (colour, point), adds the sums into counts and
 * applies the shift, the two indices and the lut, one writer per entry.  Integers only, and an integer sum does not depend on
 * the order of its terms: the result is the definition's for every input, whatever the scheduling.
 * No wrap.  A workgroup of the second launch sees at most 16 * 1024 = 2^14 plays: its LDS partial counts are uint32.  A call
 * adds at most records * playouts * max_plies <= 2^24 * 2^10 = 2^34 to an entry: the sums in scratch are uint64.  With limit >
 * 0 an entry is below limit <= 2^30 after every call, so it never exceeds 2^30 + 2^34.  With limit == 0 the counts only grow,
 * and the caller keeps played below 2^54: 64 * (2 * won + k) then stays below 2^62.
 * scratch: bkt_move_context_scratch_bytes(records) = 13,284 * 16 = 212,544 bytes on the device whatever the number of records,
 * 8-byte aligned (0 when records < 1); its contents on entry do not matter, and two updates back to back on one stream may
 * share it.
 * Domain: bkt_move_value_update's, scratch 8-byte aligned, and 1 <= min_plays <= BKT_MOVE_CONTEXT_MAX_MIN_PLAYS.  Else
 * BKT_ERR_ARG: a refused call launches nothing and writes nothing. */
#define BKT_MOVE_CONTEXT_MAX_MIN_PLAYS (1 << 30)
int bkt_move_context_playouts(void *pos, int batch, uint64_t seed, const uint32_t *counters, const uint16_t *table,
                              const uint16_t *tactics, const uint16_t *values, const uint8_t *replies, const uint8_t *replies2,
                              int max_plies, uint8_t *over, int32_t *plies, int16_t *moves, int32_t *status, void *stream);
size_t bkt_move_context_scratch_bytes(int records);
int bkt_move_context_update(const void *pos, const int16_t *moves, int max_plies, const uint8_t *won, int records, int playouts,
                            int64_t *counts, uint16_t *values, const uint16_t *lut, int k, int limit, int min_plays,
                            void *scratch, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* BOKEGO_TRAIN_H */
