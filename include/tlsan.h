/*
 * tlsan.h -- C ABI of libtlsan_hip.so: the MI355X (gfx950) TLSAN hot path.
 *
 * The reference (TsingZ0/TLSAN) has no FFI: its hot path sits behind the Python class
 * `Model` (TLSAN/model.py:13-313) whose methods call `sess.run` on a TensorFlow-1.8 graph.
 * Each entry point below replaces one such `sess.run` fetch; the Python `tlsan_amd.Model`
 * (same constructor / method surface as the reference's Model) binds them with ctypes.
 * INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer inside the structs is a DEVICE pointer unless marked "host";
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); all work is enqueued
 *     on it, nothing synchronises, nothing allocates (caller supplies `ws` and `state`);
 *   - return value: 0 = ok, negative = TLSAN_E_* (never throws across the ABI);
 *     tlsan_last_error() returns a host string for the calling thread's last failure;
 *   - single host thread per GPU, like the reference (one tf.Session, synchronous).
 */
#ifndef TLSAN_H_
#define TLSAN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TLSAN_ABI_VERSION 15

enum {
  TLSAN_OK = 0,
  TLSAN_E_BADARG = -1,      /* unsupported dims / null pointer / shape mismatch            */
  TLSAN_E_WORKSPACE = -2,   /* ws or state buffer too small                              */
  TLSAN_E_LAUNCH = -3,      /* HIP launch error (see tlsan_last_error)                   */
  TLSAN_E_UNSUPPORTED = -4  /* valid request outside what this build implements          */
};

/* Shapes: config keys read by model.py:64,72,76,81,102,116-117. */
typedef struct {
  int32_t user_count, item_count, cate_count;
  int32_t d;          /* hidden_units = d_item + d_cate = d_user + d_cate (model.py:100-109,135) */
  int32_t d_item;     /* itemid_embedding_size (== userid_embedding_size)                        */
  int32_t d_cate;     /* cateid_embedding_size                                                  */
  int32_t num_heads;  /* (d, num_heads) in {64/4, 64/8, 128/4, 128/8, 128/16, 256/8}; else UNSUPPORTED */
  int32_t Ls;         /* long-term window (columns of hist_i / usert_emb), <= 96 (reference max_length = 90) */
} tlsan_dims;

/* Trainable variables of model.py:58-81 + attention/dense weights, fp32, row-major.
 * `dense` packs the small weights (layout: tlsan_dense_layout):
 *   fwa1{W1[dh,dh],b1[dh],W2[dh,dh],b2[dh]} | K[d,d] (tf.layers.dense kernel, model.py:347) |
 *   k0[d] | fwa2{W1,b1,W2,b2} | gamma[1]
 * `dense_KT` is K transposed, maintained by the library after every update
 * (tlsan_sync_derived must be called after the caller writes `dense` itself). */
typedef struct {
  float* item_emb;            /* [I, d_item] */
  float* item_b;              /* [I]         */
  float* user_emb;            /* [U, d_item] */
  float* usert_emb;           /* [U, Ls]     */
  float* cate_emb;            /* [C, d_cate] */
  float* dense;               /* [n_dense]   */
  float* dense_KT;            /* [d, d]      */
  const int32_t* item_cate;   /* [I] item -> category (model.py:85 graph constant) */
  /* Row strides in floats; 0 = densely packed (d_item, 1, d_item, Ls).  Non-zero strides let
   * the tables alias fused rows, e.g. [item_emb | item_b | pad] as exchanged between GPUs. */
  int32_t ld_item, ld_itemb, ld_user, ld_usert;
  /* Optional DEVICE scalar P (NULL = 1): the four L2-regularised tables hold W / P, i.e. the
   * true parameters are P * stored (item_b and `dense` are never scaled).  With
   * TLSAN_L2_LAZY the library keeps P = prod_t (1 - lr_t c_t reg) here instead of decaying
   * every row every step; point it at tlsan_state_scale(state). */
  const float* scale;
  /* Storage type of item_emb, user_emb and cate_emb: TLSAN_TABLE_F32 (0) or TLSAN_TABLE_BF16 (1).
   * With bf16 the three pointers address uint16 elements (row strides still in ELEMENTS); all
   * arithmetic stays fp32, updates are written back with stochastic rounding (deterministic: a
   * hash of step, table and element).  usert_emb, item_b and dense are always fp32.  A build
   * extension: the reference is fp32 throughout. */
  int32_t table_dtype;
  /* Arithmetic of the matrix products of the fused kernel (the two maps of both attention blocks, forward and
   * backward, their weight gradients, the bridge GEMM and its transpose): TLSAN_MATRIX_F32 (0) --
   * v_mfma_f32_16x16x4_f32, exact fp32, the reference's precision; TLSAN_MATRIX_BF16 (1) -- both operands of
   * every product rounded to bfloat16 (nearest even), products and sums in fp32
   * (v_mfma_f32_16x16x16_bf16).  Everything else (softmax, loss, gradients' sums, updates) is fp32 either
   * way.  A build extension for BASELINE.json configs[2] ("bf16"); logits then agree with the fp32 oracle
   * to about 1e-2, not 1e-4. */
  int32_t matrix_dtype;
} tlsan_params;
#define TLSAN_TABLE_F32 0
#define TLSAN_TABLE_BF16 1
#define TLSAN_MATRIX_F32 0
#define TLSAN_MATRIX_BF16 1

typedef struct {
  int32_t n_dense;
  int32_t f1_W1, f1_b1, f1_W2, f1_b2, K, k0, f2_W1, f2_b1, f2_W2, f2_b2, gamma;
} tlsan_dense_layout;

/* One batch = the placeholders of model.py:27-53, int32 / fp32, as fed by
 * model.py:210-222 (train) and :239-262 (eval). */
typedef struct {
  int32_t B;                  /* rows in this batch                                     */
  int32_t Sn;                 /* columns of hist_i_new (max session length in batch)    */
  const int32_t* u;           /* [B]                                                    */
  const int32_t* i;           /* [B] candidate item (train target / eval positive)      */
  const int32_t* j;           /* [B] optional second candidate (eval negative) or NULL  */
  const float* y;             /* [B] labels (train only, may be NULL for forward)       */
  const int32_t* hist_i;      /* [B, Ls]                                                */
  const int32_t* hist_i_new;  /* [B, Sn]                                                */
  const float* hist_t;        /* [B, Ls]                                                */
  const int32_t* sl;          /* [B] valid length of hist_i  (1..Ls)                    */
  const int32_t* sl_new;      /* [B] valid length of hist_i_new (0..Sn)                 */
  const int32_t* u_cate;      /* [B]                                                    */
} tlsan_batch;

enum { TLSAN_NORM_TF18 = 0, TLSAN_NORM_DEDUP = 1 };
/* L2 term of model.py:164-172.  DENSE: every row of the four tables is decayed every step, as the
 * reference's dense gradient does.  LAZY: algebraically the same update,
 *   W <- (1 - lr c reg) W - lr c G_sparse,
 * kept as W = P * W_stored with one global scale P, so only rows that received a gradient are
 * read and written (identical up to fp32 rounding; required for tables that do not fit a
 * per-step sweep). */
enum { TLSAN_L2_DENSE = 0, TLSAN_L2_LAZY = 1 };

/* Hyper-parameters of one step: model.py:172 (regulation_rate), :201 (max_gradient_norm),
 * lr placeholder :49; optimizer = sgd (:195). */
typedef struct {
  float lr;
  float reg;
  float clip;
  int32_t norm_mode;  /* TLSAN_NORM_*: how clip_by_global_norm's norm treats repeated ids */
  int32_t l2_mode;    /* TLSAN_L2_*                                                       */
  /* The destination index of a batch (use counts, segment offsets, used-row records) depends only on
   * the batch's ids.  The state holds three index slots (0..2): index_slot picks the one this
   * step uses; index_prebuilt != 0 says tlsan_batch_index already built it (e.g. on a second stream
   * while the previous step ran), otherwise the step builds it itself.  Defaults 0, 0. */
  int32_t index_slot;
  int32_t index_prebuilt;
  /* config['dropout'] (model.py:116-118, 428-431): tf.nn.dropout with keep_prob = 1 - dropout on
   * the inputs of the two linear maps of both attention blocks, train steps only (forward / evaluation
   * never drop).  TF's random stream is not reproducible; the keep / drop pattern is a hash of
   * (dropout_seed, sample, block, position, map, channel) -- pass a different seed every step.
   * 0 = off (the reference's default).  Supported for fp32 and bf16 tables, fp32 and bf16 matrix products. */
  float dropout;
  uint32_t dropout_seed;
  uint32_t dropout_sample0;   /* position of this batch's first sample in the pattern: a rank's offset into the global batch */
} tlsan_hparams;

/* Device-side results of a train step (all optional except loss).
 *
 * Divergence: the reference's loss goes NaN when training diverges (model.py:171, printed at train.py:205) and
 * tf.clip_by_global_norm hands a non-finite norm on to every gradient.  The same holds here: a NaN or Inf in any
 * gathered row or weight reaches `loss` and `gnorm` (plain IEEE arithmetic carries it through the logit, the BCE and
 * the square sums; the fused kernel's units are built with -fno-honor-nans, which only frees the compiler from
 * canonicalising in front of fmaxf -- no comparison there decides whether a value is reported), and the clip
 * coefficient is formed so that a non-finite norm is not swallowed (clip_coef: NaN -> NaN, +Inf -> 0), i.e. the
 * step's update and the lazy table scale carry it on.  No separate "finite" flag: a caller tests the loss, as the
 * reference's driver does.  Pinned by tests/test_gpu_parity.py::test_nonfinite_inputs_give_nonfinite_loss. */
typedef struct {
  float* loss;    /* [1]  mean BCE + reg * l2 (model.py:171-172), value BEFORE the update */
  float* gnorm;   /* [1]  global gradient norm used for clipping                           */
  float* logits;  /* [B]  model.py:137 (may be NULL)                                       */
  float* sq_rows; /* [1]  sum of squares of every per-use embedding-gradient row (the sparse
                     part of TF-1.8's global norm); may be NULL                              */
  /* Optional (may be NULL; ABI 13): a word in HOST-visible memory (hipHostMalloc) into which the step's first
   * kernel stores `started_value` when it begins to run -- everything queued on the stream before the step has
   * completed by then.  A caller that must know this (to reuse an index slot on another stream) polls the word
   * instead of recording an event between two steps: an event is a barrier packet in the queue and costs the next
   * kernel ~5 us. */
  uint32_t* started;
  uint32_t started_value;
} tlsan_step_out;

int tlsan_abi_version(void);
const char* tlsan_last_error(void);

int tlsan_dense_layout_of(const tlsan_dims* dims, tlsan_dense_layout* out);

/* Bytes of scratch for batches up to (max_B, max_Sn).  Contents need not persist. */
size_t tlsan_workspace_bytes(const tlsan_dims* dims, int32_t max_B, int32_t max_Sn);

/* Bytes of persistent optimizer-side state (running sums of squares of the four
 * regularised tables for the L2 term / clip norm; scatter index counters). */
size_t tlsan_state_bytes(const tlsan_dims* dims);

/* (Re)initialise `state` from the current parameters and refresh dense_KT.  Call once
 * after creating / restoring / externally modifying parameters. */
int tlsan_state_init(const tlsan_dims* dims, const tlsan_params* p, void* state, void* stream);

/* Address (inside `state`) of the table scale P maintained by TLSAN_L2_LAZY steps. */
const float* tlsan_state_scale(const void* state);


/* Fold the scale into the tables (stored *= P, P = 1).  Call before reading the tables as plain
 * parameters (checkpoint) or when P gets small (long lazy runs: P ~ exp(-sum lr c reg)). */
int tlsan_state_renorm(const tlsan_dims* dims, const tlsan_params* p, void* state, void* stream);

/* Make the correction that the last TLSAN_L2_LAZY step may still owe (see tlsan_train_step: the two-launch form).  After it
 * the tables, the dense parameters and the scale are those of the reference's update.  One short launch, which returns
 * at once on the device when nothing is owed -- and, unless `stream` is being captured, the call then waits for the stream
 * and reads one word of the state: if a training step gave up its bounded wait for a correction (it left the scale NaN),
 * the call returns TLSAN_E_LAUNCH and tlsan_last_error says so.  That is the only place where that failure reaches the
 * host other than as a non-finite loss.  The library's own calls that read or rewrite the parameters through `state`
 * (tlsan_train_step in another form or with an index it builds itself, tlsan_grads, tlsan_state_renorm,
 * tlsan_state_reindex) flush by themselves; call it before anything that reads p's arrays without `state`: the forward
 * and the evaluation calls, a copy to the host, a checkpoint.  Between two steps whose index was built ahead
 * (tlsan_batch_index) no call is needed.
 * Captured steps (stream capture into a graph): a replay passes the host by, so what keeps replays right is in the graph.
 * A two-launch step that builds its own index records this flush in front of itself, always; one whose index was built
 * ahead corrects at the head of its fused kernel, as outside a graph.  Either way a replay after a clipped replay is
 * correct; anything ELSE that reads the parameters after a replay needs this call first. */
int tlsan_state_flush(const tlsan_dims* dims, const tlsan_params* p, void* state, void* stream);

/* Clear the use counters and rebuild the static category->items index for p->item_cate without
 * touching the sums of squares (used by callers whose item table changes every step). */
int tlsan_state_reindex(const tlsan_dims* dims, const tlsan_params* p, void* state, void* stream);

/* Rebuild only the category->items index for p->item_cate (same dims as before, use counters
 * untouched -- they are zero between steps): for callers whose item -> category map changes every
 * step while the table shape stays (the padded compact table of the sharded path). */
int tlsan_state_recategorize(const tlsan_dims* dims, const tlsan_params* p, void* state, void* stream);

/* Refresh derived copies (dense_KT) after the caller wrote p->dense. */
int tlsan_sync_derived(const tlsan_dims* dims, const tlsan_params* p, void* stream);

/* Forward only -- replaces `sess.run(self.logits)` (model.py:239-262).
 * logits_i[B] for candidate b->i; logits_j[B] for b->j when both are non-NULL;
 * u_t[B,d] (model.py:135) when non-NULL (input of tlsan_eval_ranks). */
int tlsan_forward(const tlsan_dims* dims, const tlsan_params* p, const tlsan_batch* b,
                  float* logits_i, float* logits_j, float* u_t,
                  void* ws, size_t ws_bytes, void* stream);

/* The same, and the two attention-weight tensors the reference keeps on the model (model.py:122: self.att0, self.att1 =
 * `soft` of feature_wise_attention, model.py:386-394, heads split along the batch axis) when non-NULL:
 *   att0[num_heads * B, Ls, d / num_heads]      long-term block, row h * B + b; exactly 0 past sl[b]
 *   att1[num_heads * B, 1 + Sn, d / num_heads]  short-term block, position 0 = the bridge; exactly 0 past 1 + sl_new[b]
 * One deviation, for a sample with sl[b] == 0 (an empty history: never in the reference's data, build_dataset.py:49-52):
 * the reference's softmax over a fully masked row (model.py:384-386) is the uniform 1 / Ls; here that row of att0 is 0.1
 * at every position when the window is held in registers (Ls <= 10) and exactly 0 when it is streamed (Ls > 10).  No
 * other output depends on it: the long-term vector of such a sample is 0 in the reference and here. */
int tlsan_forward_att(const tlsan_dims* dims, const tlsan_params* p, const tlsan_batch* b,
                      float* logits_i, float* logits_j, float* u_t, float* att0, float* att1,
                      void* ws, size_t ws_bytes, void* stream);

/* One optimisation step -- replaces `sess.run([self.loss, self.train_op])`
 * (model.py:208-234): forward, BCE + L2 loss, backward, global-norm clip, SGD update of
 * every trainable, deterministic (bitwise reproducible) scatter-add of the embedding
 * gradients.
 * TLSAN_L2_LAZY, how the update is issued (round 6; an implementation note, the results are those of the
 * reference's update either way): where it was measured to win the used rows are summed AND updated by one launch beside
 * the gradient finalize, with clip coefficient 1 -- clip_by_global_norm's coefficient whenever the norm does not exceed
 * the clip --, and a second launch commits the table scale, updates the dense weights and, after a clipped or non-finite
 * step only, corrects the rows (w_spec - (s_true - s_spec) g = w_old - s_true g up to one rounding: one ulp of the
 * SPECULATIVE value, which is why bf16 tables that the caches hold keep the form that waits).  Category rows that several
 * workgroups share (a few, large categories) are updated by the second launch, with the true coefficient.  Unclipped steps
 * are bit-equal to the form that waits for the coefficient.  `state` grew by 64 sum-of-squares records for it
 * (tlsan_state_bytes); nothing else in the ABI changed (TLSAN_ABI_VERSION stays 14).
 * The two-launch form (the shapes of the one-pass form without shared categories whose tables the caches hold -- tables
 * of more than 512 MB keep the second launch, where it measured faster; TLSAN_TWO_LAUNCH=0 keeps it everywhere).  A CHANGE OF BEHAVIOUR under the same ABI number, for callers that read p's arrays themselves: after a
 * clipped or non-finite step the arrays hold speculative values until the next step or a tlsan_state_flush.  A caller
 * that trains and then evaluates, copies or saves calls tlsan_state_flush in between; it costs one launch.
 * The step is k_fwd_bwd and k_finalize_update, nothing else, when its index was built ahead (hparams.index_prebuilt);
 * a step that builds its own index is preceded by the flush launch (three launches, as before) when the state's last
 * step had this form, because the correction walks the index slot that the build overwrites.  The finalize's workgroups store the dense
 * weights with coefficient 1 as they reduce their gradients and its summary commits the scale; after an unclipped step
 * -- nearly every step -- everything is committed when the stream drains.  After a clipped or non-finite step the rows and
 * the dense weights hold the speculative values and the correction is OWED: the next step of this form makes it at the
 * head of its fused kernel (the first 64 workgroups correct, every workgroup waits for them, bounded: after 2 s the scale
 * becomes NaN and so does every later loss), any other call that reaches the parameters through `state` makes it first,
 * and tlsan_state_flush makes it on request.  The step's index slot (hparams.index_slot) must not be rebuilt before that:
 * a caller that builds indices ahead on another stream (tlsan_batch_index) starts the build of a slot only after
 * tlsan_step_out.started of the step that FOLLOWS the slot's last step.  The correction also reads the owing step's
 * gradient rows and reduced dense gradients in `ws`: until the next step or flush, `ws` must be the same block, still
 * allocated, and not written by anything else (a caller that wants another workspace flushes first).  `state` grew by
 * the step's arguments for it (tlsan_state_bytes); tlsan_state_flush is an added call and no structure changed, so
 * TLSAN_ABI_VERSION stays 14 -- see the change of behaviour above. */
int tlsan_train_step(const tlsan_dims* dims, const tlsan_params* p, const tlsan_batch* b,
                     const tlsan_hparams* hp, const tlsan_step_out* out,
                     void* state, void* ws, size_t ws_bytes, void* stream);

/* The reference's other optimizers (model.py:188-193: adadelta | adam | rmsprop, TF-1.8 defaults).
 * Their per-parameter accumulators ("slots") are two more sets of tables with the shapes of
 * `tlsan_params` (fp32, own row strides; item_cate / dense_KT / scale / table_dtype are ignored):
 *   ADAM     (beta1 0.9, beta2 0.999, epsilon 1e-8):  slot1 = m, slot2 = v, zero-initialised;
 *            `step` = number of this update counted from 1 (the beta powers);
 *   RMSPROP  (beta1 = decay 0.9, beta2 = momentum 0.0, epsilon 1e-10): slot1 = rms (initialised
 *            to ONE as TF does), slot2 = momentum (zero);
 *   ADADELTA (beta1 = rho 0.95, epsilon 1e-8): slot1 = accum, slot2 = accum_update (zero).
 * Arithmetic of TF 1.8's training ops (core/kernels/training_ops.cc ApplyAdam / ApplyRMSProp /
 * ApplyAdadelta and their Sparse* forms).  The embedding gradients reach the optimizer as
 * IndexedSlices covering every row (gathers + the dense L2 term), so every row of the four
 * regularised tables is updated every step; item_b (not regularised) is updated where used
 * (RMSProp, Adadelta) or everywhere (Adam, whose sparse form decays m and v of all rows).
 * Needs hp->l2_mode == TLSAN_L2_DENSE; fp32 slots (the tables may be bf16).  kind == TLSAN_OPT_SGD (or opt == NULL) is
 * tlsan_train_step.
 *
 * kind | TLSAN_OPT_LAZY (ADAM, RMSPROP or ADADELTA; the "lazy" / sparse optimizers of TF's LazyAdamOptimizer and
 * torch.optim.SparseAdam): the dense step of the same optimizer, from the same parameters and slots, RESTRICTED to the
 * rows the batch used.  Same constructor defaults, slots and slot initialisation as the dense kind.
 *   - loss and clip norm: the dense optimizer's (L2 term over the whole tables, TF18 norm, formed as the lazy-L2 SGD step
 *     forms them): the clip coefficient c is the dense one up to summation order;
 *   - a used row gets the dense update with its slots, g = c * (sum of its uses' gradients + reg * W), as a whole row
 *     (usert_emb: all Ls columns).  Used: user rows of b->u; item rows of the candidates b->i and of the valid positions of
 *     hist_i (< sl) and hist_i_new (< sl_new); category rows of a u_cate, or of the item at a used position -- a category
 *     row moves when the index counts a u_cate use of it (with category segments: any use) or when its summed gradient has
 *     a non-zero element; padding is not a use;
 *   - item_b (not regularised) moves where its summed gradient is non-zero: the candidates (a candidate whose sigmoid
 *     saturates to exactly y has gradient 0 and keeps its slots, as under the dense RMSProp / Adadelta);
 *   - EVERY OTHER ROW keeps W and both slots bit for bit: the L2 term of unused rows counts in the loss and the norm but
 *     does not reach the update.  This is the intended deviation from the dense forms;
 *   - the dense weights move every step, as under the dense optimizer;
 *   - the step does not change the table scale P.  On a fresh state P is 1 and stays exactly 1 (the stored tables are
 *     the parameters; St stays their sum of squares).  If lazy-L2 SGD steps ran on the same state before (P != 1), the
 *     step acts on the true values P * stored, as the forward pass and the loss do, and stores (P * w)' / P.
 * Needs hp->l2_mode == TLSAN_L2_LAZY, norm_mode TLSAN_NORM_TF18 and params->scale == tlsan_state_scale(state)
 * (TLSAN_E_UNSUPPORTED / TLSAN_E_BADARG otherwise, before any launch); bf16 tables, dropout and matrix_dtype as usual.
 * TLSAN_OPT_LAZY alone (or with SGD) is TLSAN_E_BADARG.  An index prebuilt with TLSAN_INDEX_FOR_LAZY_SGD serves these
 * steps too.  The row launch reads the summed gradient, W, m and v of the used rows and writes W, m and v: seven row
 * widths per used row, where the lazy SGD update moves three (category rows: every row's summed gradient is read, W, m
 * and v of the used ones only).
 *
 * TLSAN_OPT_ADAGRAD | TLSAN_OPT_LAZY and TLSAN_OPT_ROWWISE_ADAGRAD | TLSAN_OPT_LAZY: Adagrad on the used rows, with ONE
 * accumulator -- slot1; slot2 is never read or written and may be NULL.  Everything above holds for them (used rows,
 * item_b, dense weights, unused rows and their accumulators bit for bit, P, the contract) but the rule, which is TF 1.8's
 * ApplyAdagrad:  acc += g^2;  w -= lr * g / sqrt(acc).  No epsilon; beta1, beta2, epsilon and step are not looked at.  The
 * library never initialises slots: TF's initial_accumulator_value is 0.1.
 *   ADAGRAD          (TF's AdagradOptimizer): an accumulator per element; slot1 has the shapes of the parameters.
 *   ROWWISE_ADAGRAD  (the row-wise Adagrad of DLRM / FBGEMM / TorchRec): an accumulator per table ROW.
 *            slot1->item_emb, user_emb, usert_emb and cate_emb are contiguous arrays of one float per row ([item_count],
 *            [user_count], [user_count], [cate_count]; their ld_* fields are not looked at, no stride rule).  For a used
 *            row of n live columns (item_emb, user_emb: d_item; usert_emb: Ls; cate_emb: d_cate)
 *              acc_row += (1 / n) * sum_j g_j^2;  w_j -= lr * g_j / sqrt(acc_row) for every j, with the new acc_row.
 *            user_emb and usert_emb are two variables with an accumulator each.  item_b and the dense weights have width 1
 *            and take the elementwise rule (slot1->item_b, slot1->dense as under ADAGRAD): on a row of width 1 the two
 *            kinds are the same arithmetic.  The row sum has a fixed order (each of the row's 16 lanes adds the squares of
 *            its own columns in ascending order, then a four-step butterfly): two runs leave the same bits.
 *            The row launch moves three row widths and one float per used row and table.
 * Both are valid only with TLSAN_OPT_LAZY: without it TLSAN_E_UNSUPPORTED, before any launch (the dense sweep is not built
 * for them).  A NULL slot1, or a NULL table in it, is TLSAN_E_BADARG.  The tlsan_shard_* calls do not take them. */
enum { TLSAN_OPT_SGD = 0, TLSAN_OPT_ADAM = 1, TLSAN_OPT_RMSPROP = 2, TLSAN_OPT_ADADELTA = 3,
       TLSAN_OPT_ADAGRAD = 4, TLSAN_OPT_ROWWISE_ADAGRAD = 5 };
#define TLSAN_OPT_LAZY 0x100
typedef struct {
  int32_t kind;
  int32_t step;
  float beta1, beta2, epsilon;
  const tlsan_params* slot1;
  const tlsan_params* slot2;
} tlsan_optimizer;
int tlsan_train_step_opt(const tlsan_dims* dims, const tlsan_params* p, const tlsan_batch* b,
                         const tlsan_hparams* hp, const tlsan_optimizer* opt, const tlsan_step_out* out,
                         void* state, void* ws, size_t ws_bytes, void* stream);

/* Device-resident batcher.  A sample set packed as CSR, every pointer a DEVICE
 * pointer (counterpart of the python lists `dataset.pkl` holds, build_dataset.py:58-59,71):
 * sample s has history hist[hist_off[s] .. hist_off[s+1]) with weights hist_t (same indexing),
 * current session sess[sess_off[s] .. sess_off[s+1]), user u[s], category cate[s],
 * target[s] = the candidate (train) / positive (test) item, second[s] = the 0/1 label (train) /
 * the negative item (test). */
typedef struct {
  int32_t n;
  const int32_t* u; const int32_t* cate;
  const int32_t* hist_off; const int32_t* hist; const float* hist_t;
  const int32_t* sess_off; const int32_t* sess;
  const int32_t* target; const int32_t* second;
} tlsan_packed;

/* tlsan_batch_pack -- replaces DataInput.__next__ / DataInputTest.__next__ (TLSAN/input.py:17-54,
 * 70-107) without touching the host: assemble samples order[lo .. lo + out->B) of `set` into the
 * caller-allocated device arrays of `out` (u, i, y (train) or j (test), hist_i [B,Ls],
 * hist_i_new [B,Sn], hist_t [B,Ls], sl, sl_new, u_cate).  out->Sn must be >= the longest session
 * of the batch (the reference pads to exactly the longest; pass that for identical shapes).
 * Bit-identical to the reference's arrays on the committed fixtures. */
int tlsan_batch_pack(const tlsan_packed* set, const int32_t* order, int32_t lo, const tlsan_batch* out,
                     int32_t Ls, int32_t is_test, void* stream);

/* Build the destination index of batch `b` into index slot `slot` (0 .. 2) of the state: the two
 * launches a step otherwise starts with.  Independent of the parameters, so an input pipeline can
 * run it for the next batches on another stream while the current step computes; the caller orders
 * it after the last step that used the same slot and before the step that consumes it.
 * slot | TLSAN_INDEX_FOR_LAZY_SGD: the index will be consumed by a lazy-L2 SGD train step only, which reaches the
 * user table's offsets through the batch's ids and the used-row records -- they are then written for the used rows
 * only (10 M users: 80 MB less per step).  An index built that way must not feed tlsan_grads or a dense-L2 step; it does
 * serve a lazy optimizer's step (tlsan_optimizer, TLSAN_OPT_LAZY), which walks the same records.
 * item_cate: params->item_cate of the tables the step will run on (tables with thousands of categories count item
 * uses per category as well; may be NULL below TLSAN_CSEG_MIN categories -- the only parameter-side input, and it is
 * not a trainable). */
#define TLSAN_INDEX_FOR_LAZY_SGD 0x100
int tlsan_batch_index(const tlsan_dims* dims, const tlsan_batch* b, const int32_t* item_cate, void* state, int32_t slot,
                      void* stream);

/* For tests and tools (ABI 15): a read-only view of an index slot and of the form it is built in.  Host-only: both calls
 * launch nothing and touch no device memory.  Nothing in the product calls them.
 *
 * tlsan_index_layout_of: where the destination index of slot `slot` (0 .. 2) lives inside the state buffer, as BYTE
 * OFFSETS from the state's first byte (the caller slices its own buffer), from the one definition of the state's layout.
 * All arrays are int32 but the records (four int32 each: row, first position, uses, 0):
 *   cnt_item [I], cnt_uc [C], cnt_user [U]     use counters, zero at rest (a build adds, the consuming step counts back)
 *   off_*    [n + 1]                           first sorted position of every row, off[n] = all uses
 *   cur_*    [n]                               fill cursors (== off after a build; cur_uc is advanced by the category lists)
 *   urec_item, urec_user                       records of the used rows, ascending by row
 *   perm     [rank_cap]                        the batch's ranking for the fused kernel's workgroups (16 places per group)
 *   uc_list  [uc_list_cap]                     the samples of every category, category c at [off_uc[c], off_uc[c + 1])
 *   hot_list [ap_hot_cap]                      record slots (urec_item) of the item rows with more than ap_hot uses
 *   flag_user [ceil(U / 256)]                  marks of the 256-row pieces of the user counters, zero at rest
 *   scan_ticket [3]                            arrival counters of the scan, one per slot (the same offset for every slot), zero at rest
 *   n_uniq, n_hot                              the header's words of the slot: used rows [item, user] (two int32), hot rows */
typedef struct {
  int64_t cnt_item, cnt_uc, cnt_user;
  int64_t off_item, off_uc, off_user;
  int64_t cur_item, cur_uc, cur_user;
  int64_t urec_item, urec_user;
  int64_t perm, uc_list, hot_list, flag_user;
  int64_t scan_ticket;
  int64_t n_uniq, n_hot;
  int32_t rank_cap, uc_list_cap;
  int32_t ap_hot, ap_hot_cap;
} tlsan_index_layout;
int tlsan_index_layout_of(const tlsan_dims* dims, int32_t slot, tlsan_index_layout* out);

/* tlsan_index_plan_of: the form tlsan_batch_index builds the index in for a batch of B samples with Sn session columns;
 * flags: 0 or TLSAN_INDEX_FOR_LAZY_SGD.  Reads only these numbers and the dims (and the library's environment switches). */
typedef struct {
  int32_t cseg;        /* category segments: item uses are counted into their item's category as well */
  int32_t uc_list;     /* the samples of every category are listed */
  int32_t usort;       /* the user side comes from a sort of the batch's ids: no user counters */
  int32_t isort;       /* the item side comes from a partitioned counting sort: no item counters */
  int32_t sparse;      /* bit t (0 item, 1 category, 2 user): off / cur of that table are written for the used rows only */
  int32_t rank;        /* a ranking of the batch is written */
  int32_t by_window;   /* ... keyed by window length (> 0) or by session and window (0) */
  int32_t two_level;   /* the scan takes its two-launch form (a table of more than 16 chunks of 4096 rows) */
} tlsan_index_plan;
int tlsan_index_plan_of(const tlsan_dims* dims, int32_t B, int32_t Sn, int32_t flags, tlsan_index_plan* out);

/* Gradients only (no update) -- what `tf.gradients(self.loss, trainables)` (model.py:198)
 * returns, with duplicate ids summed and reg*W added for the four regularised tables.
 * Used by the parity tests.  Each output has the shape of the parameter it mirrors. */
typedef struct {
  float* item_emb; float* item_b; float* user_emb; float* usert_emb; float* cate_emb;
  float* dense;    /* [n_dense] */
  /* row strides in floats of the four row outputs; 0 = packed (d_item, 1, d_item, Ls) */
  int32_t ld_item, ld_itemb, ld_user, ld_usert;
  /* != 0: rows that received no gradient are not written (the caller zeroed the buffers).  With
   * strides this lets item and user gradients land in ONE fused [rows, W] buffer when a row is
   * only ever used as one kind (the compact per-step table of the sharded path).
   * 2 (with hp->reg == 0 and the tf18 norm, the pure row-sum path): the four row outputs ARE one fused
   * table of rows [item_emb | item_b | pad] / [user_emb | usert_emb | pad] of width ld_item == ld_user;
   * a written row is written in full (its unowned tail cleared), so only rows that received no
   * gradient keep the caller's content -- the buffer need not be zeroed when every row sent on is used. */
  int32_t sparse;
} tlsan_grads_out;
int tlsan_grads(const tlsan_dims* dims, const tlsan_params* p, const tlsan_batch* b,
                const tlsan_hparams* hp, const tlsan_grads_out* g, const tlsan_step_out* out,
                void* state, void* ws, size_t ws_bytes, void* stream);

/* All-items scoring -- replaces the metric update ops on `eval_logits`
 * (model.py:140-156): for each row, the rank of `labels[b]` inside
 * u_t[b] . [item_emb || cate_emb[item_cate]]^T + item_b under tf.nn.top_k's order
 * (higher score first, ties -> lower item id first).  hit@k == (rank < k).
 * The [B, I] score matrix is never materialised. */
int tlsan_eval_ranks(const tlsan_dims* dims, const tlsan_params* p, const float* u_t,
                     const int32_t* labels, int32_t B, int32_t* ranks,
                     void* ws, size_t ws_bytes, void* stream);

/* Item-sharded all-items scoring (the evaluation half of the multi-GPU path):
 *   tlsan_eval_label_scores: scores[b] = u_t[b] . all_emb[labels[b]] + item_b[labels[b]] on a table that
 *     holds the label rows (the rank that owns the users: its compact per-step table);
 *   tlsan_eval_counts_shard: for every row of u_t (the users of ALL ranks, all-gathered) the number
 *     of items of THIS rank's shard ranked ahead of the label under tf.nn.top_k's order; local item n
 *     is global item n * id_mul + id_add (ties -> lower GLOBAL id first).  Summing the counts over
 *     the ranks gives tlsan_eval_ranks' result on the unsharded table. */
int tlsan_eval_label_scores(const tlsan_dims* dims, const tlsan_params* p, const float* u_t, const int32_t* labels,
                            int32_t B, float* scores, void* ws, size_t ws_bytes, void* stream);
int tlsan_eval_counts_shard(const tlsan_dims* dims, const tlsan_params* p, const float* u_t, const float* label_scores,
                            const int32_t* labels_global, int32_t B, int32_t id_mul, int32_t id_add, int32_t* counts,
                            void* ws, size_t ws_bytes, void* stream);

/* The all-items ranking with per-row exclusion lists: the rank of a label among the items its row has NOT seen (the
 * leave-one-out protocol of a next-item recommender).  tlsan_eval_ranks_excl / tlsan_eval_counts_shard_excl do what
 * tlsan_eval_ranks / tlsan_eval_counts_shard do -- ranks / counts are theirs, unfiltered, bit for bit -- and, in the same
 * call (one dense item matrix, where the rank path builds one, for both), say what the lists change:
 *   excl_off [B + 1] / excl_ids: row b's list excl_ids[excl_off[b] .. excl_off[b+1]) of global ids, ascending, as
 *     tlsan_eval_topk's; repeats and ids outside the table are ignored.  THE LABEL IS NEVER EXCLUDED, even when its row
 *     lists it (a test label can sit in its user's own history: SURVEY 8c).
 *   held[b]:  the number of DISTINCT listed items, other than the label, that this table holds;
 *   ahead[b]: how many of those the rank path counted ahead of the label: score > label's score, or equal and a lower
 *     global id -- the decision of the counting kernel this call ran on this table, on the same operands, the same
 *     MFMA chain and the same rounding of (acc * P) + bias (the kernel that reads the dense item matrix contracts the
 *     two into one fused multiply-add, the gathering one does not; the count of the listed items follows whichever ran).
 *   filtered rank = ranks[b] - ahead[b] (never negative);  eligible items = item_count - 1 - held[b].
 * Item-sharded form: ids this table does not hold are skipped, so counts, ahead and held each sum exactly over the ranks.
 * ranks / counts, ahead, held: [B] int32, all required.  A row's result does not depend on B, on the other rows or on
 * the launch geometry.  Workspace: tlsan_workspace_bytes(dims, B, 0), as tlsan_eval_ranks. */
int tlsan_eval_ranks_excl(const tlsan_dims* dims, const tlsan_params* p, const float* u_t, const int32_t* labels, int32_t B,
                          const int32_t* excl_off, const int32_t* excl_ids, int32_t* ranks, int32_t* ahead, int32_t* held,
                          void* ws, size_t ws_bytes, void* stream);
int tlsan_eval_counts_shard_excl(const tlsan_dims* dims, const tlsan_params* p, const float* u_t, const float* label_scores,
                                 const int32_t* labels_global, int32_t B, int32_t id_mul, int32_t id_add,
                                 const int32_t* excl_off, const int32_t* excl_ids, int32_t* counts, int32_t* ahead,
                                 int32_t* held, void* ws, size_t ws_bytes, void* stream);

/* Top-K recommendation over all items -- what the reference gets with tf.nn.top_k(eval_logits, K)
 * (model.py:140), without materialising the [B, I] scores: for each row b of u_t [B, d], the K items
 * of highest score  u_t[b] . [item_emb || cate_emb[item_cate]][n] + item_b[n]  (the scores of
 * tlsan_eval_ranks / tlsan_eval_label_scores, bit for bit), in tf.nn.top_k's order: higher score first,
 * equal scores -> lower GLOBAL id first; +0.0 == -0.0 (a zero score is returned as +0.0); a NaN score
 * ranks after every other score.  1 <= K <= 256.
 *   ids [B, K] int32, scores [B, K] float32; rows with fewer than K eligible items end in id -1, score -inf.
 *   excl_off [B + 1] / excl_ids (both NULL: no exclusion): row b's list excl_ids[excl_off[b] .. excl_off[b+1])
 *     of global ids, ascending; those items never appear in the row (ids outside the table or repeated are
 *     ignored).
 *   Item-sharded form: local item n is global id n * id_mul + id_add (1 and 0 for a whole table), as in
 *     tlsan_eval_counts_shard; the ranks' lists of a row merge with tlsan_topk_merge.
 * The result does not depend on B, on the other rows of the launch or on the launch geometry.
 * Workspace: tlsan_topk_workspace_bytes (0, with tlsan_last_error set, for bad dims / K / B). */
size_t tlsan_topk_workspace_bytes(const tlsan_dims* dims, int32_t B, int32_t K);
int tlsan_eval_topk(const tlsan_dims* dims, const tlsan_params* p, const float* u_t, int32_t B, int32_t K,
                    const int32_t* excl_off, const int32_t* excl_ids, int32_t id_mul, int32_t id_add,
                    int32_t* ids, float* scores, void* ws, size_t ws_bytes, void* stream);
/* [B, n_lists, K] lists, each sorted in that order and holding disjoint items (padded with id -1) -> the
 * [B, K] best of each row.  The merge tlsan_eval_topk runs on its item slices. */
int tlsan_topk_merge(const int32_t* cand_ids, const float* cand_scores, int32_t B, int32_t n_lists, int32_t K,
                     int32_t* ids, float* scores, void* stream);

/* Similar-items lists ("more like this"): for each query item the K nearest items of the table by the representation
 * the model scores with,  w_n = [item_emb[n] || cate_emb[item_cate[n]]]  (d columns; bf16 tables widened exactly to
 * fp32), without materialising the [Q, I] similarities.  No user context, no forward pass, no bias.  With
 *   acc(q, n) the fp32 MFMA accumulation of w_q . w_n on STORED values, in the k-order and instruction chain of
 *     tlsan_eval_topk's tiles,
 *   inv(n) = 1 / sqrtf(ss_n),  ss_n = sum_k w_n[k]^2  in fp32 in one fixed order that does not depend on the launch
 *     (0 when ss_n == 0), computed by one device function for queries and table items alike,
 *   P the table scale (*p->scale; 1 when NULL),
 * the score of item n for query q is
 *   TLSAN_SIM_DOT:     s = fl(acc * fl(P * P))             -- the product of the true vectors
 *   TLSAN_SIM_COSINE:  s = fl(acc * fl(inv(q) * inv(n)))   -- P cancels and is not applied
 * Both are symmetric in bits: s(a, b) and s(b, a) are the same float, as are the scores of bit-identical rows.
 * Order: tlsan_eval_topk's -- higher score first, equal scores -> lower GLOBAL id first; +0.0 == -0.0 (a zero score is
 * returned as +0.0); a NaN score ranks after every other score.  1 <= K <= 256.
 *
 * tlsan_item_vectors: vec[q] = w of item ids[q] and inv_norm[q] = inv of it (inv_norm may be NULL), for every id this
 *   table holds: local item n is global id n * id_mul + id_add (1 and 0 for a whole table), as in
 *   tlsan_eval_counts_shard.  Ids the table does not hold, and negative ids, get ZEROS in both, so that the results of
 *   the ranks of a sharded table combine (exactly one rank holds an id).  vec [Q, d] float32, inv_norm [Q].
 *
 * tlsan_similar_topk: ids [Q, K] int32 (global), scores [Q, K] float32 for the queries
 *   qvec [Q, d] / qinv [Q]: what tlsan_item_vectors wrote (qinv may be NULL for TLSAN_SIM_DOT); qids [Q]: their global
 *   ids.  The query item never appears in its own list.  A row with qids[q] < 0 is padding -- all id -1, score -inf --
 *   and so is, in the whole-table form (id_mul == 1, id_add == 0), a row with qids[q] >= item_count.
 *   excl_off [Q + 1] / excl_ids (both NULL: none): row q's list excl_ids[excl_off[q] .. excl_off[q+1]) of global ids,
 *     ascending, tlsan_eval_topk's format; those items never appear in the row (repeats and ids outside the table are
 *     ignored).
 *   Rows with fewer than K eligible items end in id -1, score -inf.
 *   Item-sharded form: every rank passes the same queries and its own table; the ranks' lists of a row merge with
 *     tlsan_topk_merge.
 *   A row's result does not depend on Q, on the other rows, on the launch geometry or on the number of ranks.
 * Neither call changes the parameters, P or any state.  A sum of squares that overflows fp32 has inv 0.
 * Workspace: tlsan_similar_workspace_bytes (0, with tlsan_last_error set, for bad dims / K / Q).  Refused before any
 * launch, with the function's name in tlsan_last_error: NULL pointers, K outside 1..256, Q < 1, an unknown metric, bad
 * dims (TLSAN_E_BADARG / TLSAN_E_UNSUPPORTED as everywhere), a workspace that is NULL or too small (TLSAN_E_WORKSPACE).
 * The three functions and the two constants are additions: nothing else in the ABI changed (TLSAN_ABI_VERSION stays 14). */
#define TLSAN_SIM_DOT 0
#define TLSAN_SIM_COSINE 1
int tlsan_item_vectors(const tlsan_dims* dims, const tlsan_params* p, const int32_t* ids, int32_t Q, int32_t id_mul,
                       int32_t id_add, float* vec, float* inv_norm, void* stream);
size_t tlsan_similar_workspace_bytes(const tlsan_dims* dims, int32_t Q, int32_t K);
int tlsan_similar_topk(const tlsan_dims* dims, const tlsan_params* p, const float* qvec, const float* qinv,
                       const int32_t* qids, int32_t Q, int32_t K, int32_t metric, const int32_t* excl_off,
                       const int32_t* excl_ids, int32_t id_mul, int32_t id_add, int32_t* ids, float* scores, void* ws,
                       size_t ws_bytes, void* stream);

/* Scoped lists: tlsan_eval_topk and tlsan_similar_topk over a SUBSET of the table's items, with an optional category
 * wanted per row ("the best K within these items", "more from this department").  Everything the unscoped calls say
 * about scores, order, K, the exclusion lists, padding rows, short rows and the item-sharded form holds unchanged; the
 * scores of a (row, item) pair are theirs bit for bit, and so are tlsan_eval_label_scores' and tlsan_score_candidates'.
 *   sub [nsub] / nsub: the scope, LOCAL item indices of this table (global id = sub[n] * id_mul + id_add), ascending
 *     and distinct, 0 <= nsub <= item_count; sub NULL with nsub < 0: every item of the table.  Only the scope's items
 *     are scored: the work is that of nsub items, not of item_count.  nsub == 0: every row comes back id -1, score -inf.
 *     An index outside [0, item_count) is never read as a table row and never selected (the rest of the list counts as
 *     if it were not there).  The order and distinctness of sub are the caller's to keep: they are not checked, and a
 *     repeated index can appear twice in a list.
 *   row_cate [B] (tlsan_similar_topk_scoped: [Q]) or NULL: row b selects item n only when row_cate[b] < 0 or
 *     p->item_cate[n] == row_cate[b].  A category no item of the scope has gives an all -1 / -inf row.  The category
 *     test narrows what is selected, not what is scored: without sub the whole table is still scanned.
 *   No dense [item_count, d] matrix is built, whatever the table's size.
 *   A row's result does not depend on B (Q), on the other rows, on the launch geometry or on the number of ranks: in
 *     the item-sharded form every rank passes the scope's items ITS table holds and the ranks' lists merge with
 *     tlsan_topk_merge.
 * Neither call changes the parameters, P or any state.
 * Workspace: tlsan_scope_workspace_bytes, for both calls (0, with tlsan_last_error set, for bad dims / K / B, or nsub >
 * item_count).  Refused before any launch, with the function's name in tlsan_last_error: what the unscoped call refuses,
 * with its code; sub NULL with nsub >= 0, sub given with nsub < 0, nsub > item_count (TLSAN_E_BADARG); a workspace that
 * is NULL or too small (TLSAN_E_WORKSPACE).  The three functions are additions: nothing else in the ABI changed
 * (TLSAN_ABI_VERSION stays 15). */
size_t tlsan_scope_workspace_bytes(const tlsan_dims* dims, int32_t B, int32_t K, int32_t nsub);
int tlsan_eval_topk_scoped(const tlsan_dims* dims, const tlsan_params* p, const float* u_t, int32_t B, int32_t K,
                           const int32_t* excl_off, const int32_t* excl_ids, const int32_t* sub, int32_t nsub,
                           const int32_t* row_cate, int32_t id_mul, int32_t id_add, int32_t* ids, float* scores, void* ws,
                           size_t ws_bytes, void* stream);
int tlsan_similar_topk_scoped(const tlsan_dims* dims, const tlsan_params* p, const float* qvec, const float* qinv,
                              const int32_t* qids, int32_t Q, int32_t K, int32_t metric, const int32_t* excl_off,
                              const int32_t* excl_ids, const int32_t* sub, int32_t nsub, const int32_t* row_cate,
                              int32_t id_mul, int32_t id_add, int32_t* ids, float* scores, void* ws, size_t ws_bytes,
                              void* stream);

/* Indexed lists: the scoped lists over an INDEX of the table's items -- a caller's lists of local item indices, one per
 * category (or per cell of any other partition) -- where every row names the few lists it wants.  Only those lists are
 * scored: a row costs what its lists' items cost, where tlsan_eval_topk_scoped's row_cate still scans the whole scope.
 *   list_off [nlists + 1], list_items: list c is list_items[list_off[c] .. list_off[c + 1]), LOCAL item indices of this
 *     table (global id = index * id_mul + id_add); the lists are disjoint.  An entry outside [0, item_count) is never
 *     read as a table row and never selected.  An empty list is allowed.
 *   max_list: the longest list's length as the host knows it.  It sizes the launch (the slices of a list) and the
 *     workspace, nothing else: a wrong value costs time, not correctness.  The workspace call and the list call take
 *     the same (B, P, K, nlists, max_list).
 *   row_lists [B, P] (tlsan_similar_topk_lists: [Q, P]), 1 <= P <= 8: the lists row b probes.  A negative entry, or one
 *     >= nlists (never used to address list_off), is no probe; a list named twice in a row counts once.
 *   Row b's result: the K best, in tlsan_eval_topk's order, of the union of its probed lists minus its exclusion list
 *     (and, in the similar form, minus the query itself, as tlsan_similar_topk).  A row without a probe, or with empty
 *     lists only, comes back id -1, score -inf.  The scores of a (row, item) pair are tlsan_eval_topk_scoped's /
 *     tlsan_similar_topk_scoped's bit for bit.
 *   A row's result depends on its own inputs only: not on B, on the other rows, on how the call groups the rows that
 *     share a list (it does so on the device, in the workspace, without a host synchronisation, and the grouping may
 *     differ from call to call), on the launch geometry or on the number of ranks.  In the item-sharded form every
 *     rank passes the index of ITS table's items and the ranks' lists merge with tlsan_topk_merge.
 * Neither call changes the parameters, P or any state; no dense [item_count, d] matrix is built.
 * Workspace: tlsan_lists_workspace_bytes, for both calls (0, with tlsan_last_error set, on a refusal).  Refused before
 * any launch, with the function's name in tlsan_last_error: bad dims or parameters (the unscoped call's codes); K outside
 * 1..256, P outside 1..8, B (Q) or nlists outside 1..2^24, max_list < 0, a NULL pointer, excl_off without excl_ids, an id mapping
 * that leaves int32, a metric that is none (TLSAN_E_BADARG); a workspace that is NULL or too small (TLSAN_E_WORKSPACE).
 * The three functions are additions: nothing else in the ABI changed (TLSAN_ABI_VERSION stays 15). */
size_t tlsan_lists_workspace_bytes(const tlsan_dims* dims, int32_t B, int32_t P, int32_t K, int32_t nlists, int32_t max_list);
int tlsan_eval_topk_lists(const tlsan_dims* dims, const tlsan_params* p, const float* u_t, int32_t B, int32_t K,
                          const int32_t* excl_off, const int32_t* excl_ids, const int32_t* list_off,
                          const int32_t* list_items, int32_t nlists, int32_t max_list, const int32_t* row_lists, int32_t P,
                          int32_t id_mul, int32_t id_add, int32_t* ids, float* scores, void* ws, size_t ws_bytes,
                          void* stream);
int tlsan_similar_topk_lists(const tlsan_dims* dims, const tlsan_params* p, const float* qvec, const float* qinv,
                             const int32_t* qids, int32_t Q, int32_t K, int32_t metric, const int32_t* excl_off,
                             const int32_t* excl_ids, const int32_t* list_off, const int32_t* list_items, int32_t nlists,
                             int32_t max_list, const int32_t* row_lists, int32_t P, int32_t id_mul, int32_t id_add,
                             int32_t* ids, float* scores, void* ws, size_t ws_bytes, void* stream);

/* Category shelves: for each row the S lists of an index (the indexed lists' list_off / list_items, above) whose own
 * m-lists rank highest, with those m-lists -- a page of departments and what goes on each shelf -- in one scan of the
 * index.  No [B, item_count] score array and no [B, nlists, m] array is ever built.
 *   L(b, c): the m best items of list c for row b minus the row's exclusion list, in tlsan_eval_topk's order: exactly
 *     row b of tlsan_eval_topk_lists with K = m and row_lists[b] = c, ids and score bits.  n(b, c): its valid entries.
 *   List c is a CANDIDATE of row b when no entry of skip[b, 0 .. X) names it (skip [B, X] list ids, 0 <= X <= 8, NULL
 *     with X = 0; a negative entry names nothing) and n(b, c) >= min_items, 1 <= min_items <= m.  Its rank key is entry
 *     rank_at of L(b, c), 0 <= rank_at < min_items: (score, global id) in tlsan_eval_topk's order, so NaN ranks last and
 *     +0.0 == -0.0; no arithmetic is done on scores.  Row b's page is its S candidates of highest rank key, in that order;
 *     equal rank keys (possible only when two lists hold the same item) go to the lower list id.
 *   cats [B, S], ids [B, S, m], scores [B, S, m]: shelf j of row b is list cats[b, j] with L(b, cats[b, j]).  A row with
 *     fewer than S candidates ends in cats -1, ids -1, scores -inf; entries of a shelf past n(b, c) are -1 / -inf.
 *   1 <= S <= 32, 1 <= m <= 64, S * m <= 256 (a page flattened to [B, S * m] is a list tlsan_list_metrics takes).
 *   The PLAN, built by the host from the lists' lengths, says how the scan walks the index; every list with items appears
 *     in it exactly once:
 *       seg_off [nseg + 1], seg_lists [nsmall]: segment s is the lists seg_lists[seg_off[s] .. seg_off[s + 1]); one
 *         workgroup per 16 rows walks a segment's lists one after another;
 *       big_off [nbig + 1], big_slices [nbs, 3] = (list, lo, hi): big list j is cut into the slices big_off[j] ..
 *         big_off[j + 1], at most 16, slice t the positions lo .. hi of its list; one workgroup per 16 rows and slice.
 *     The result does not depend on the plan: not on which lists share a segment, which are big or where they are cut.  A
 *     list id outside [0, nlists) or positions outside the list are passed over, never used as addresses; a list the plan
 *     leaves out is no candidate.  max_list is the longest list's length as the host knows it (>= 0; it sizes nothing).
 *   A row's result depends on its own inputs only: not on B, the other rows, a repeated call or the launch geometry.
 *   id_mul / id_add: the table's id mapping, as everywhere (the returned ids and the exclusion lists are global ids).
 * Two launches on `stream`, no host synchronisation; no grid is sized by a device value.  The call changes no parameter
 * and no state.  Workspace: tlsan_shelves_workspace_bytes(dims, B, S, m, nseg, nbig, nbs), never less for a larger
 * argument; 0, with tlsan_last_error set, on a refusal.  Refused before any launch, with the function's name in
 * tlsan_last_error: bad dims or parameters (tlsan_eval_topk_lists' codes); B or nlists outside 1..2^24, S outside 1..32,
 * m outside 1..64, S * m > 256, min_items outside 1..m, rank_at outside 0..min_items - 1, nseg or nbig outside 0..32767,
 * nbs outside nbig..min(32767, 16 nbig), nsmall < 0 (or 0 with segments), max_list < 0, X outside 0..8 or skip not going
 * with it, a NULL pointer (the plan's arrays may be NULL where their count is 0), excl_off without excl_ids, an id
 * mapping that leaves int32 (TLSAN_E_BADARG); a workspace that is NULL or too small (TLSAN_E_WORKSPACE).
 * The two functions are additions: nothing else in the ABI changed (TLSAN_ABI_VERSION stays 15). */
size_t tlsan_shelves_workspace_bytes(const tlsan_dims* dims, int32_t B, int32_t S, int32_t m, int32_t nseg, int32_t nbig,
                                     int32_t nbs);
int tlsan_eval_shelves(const tlsan_dims* dims, const tlsan_params* p, const float* u_t, int32_t B, int32_t S, int32_t m,
                       int32_t min_items, int32_t rank_at, const int32_t* excl_off, const int32_t* excl_ids,
                       const int32_t* list_off, const int32_t* list_items, int32_t nlists, int32_t max_list,
                       const int32_t* seg_off, const int32_t* seg_lists, int32_t nseg, int32_t nsmall, const int32_t* big_off,
                       const int32_t* big_slices, int32_t nbig, int32_t nbs, const int32_t* skip, int32_t X, int32_t id_mul,
                       int32_t id_add, int32_t* cats, int32_t* ids, float* scores, void* ws, size_t ws_bytes, void* stream);

/* Explanations: the exact parts of a listed score, per source ("because you viewed X").  TLSAN's logit is linear in
 * everything behind its two softmaxes, so with the attention weights taken as given (att0 / att1 exactly as
 * tlsan_forward_att writes them, row h * B + b) the score of row b for item g splits, with no gradient and no approximation,
 * into (true parameters: the four regularised tables are P * stored; names of oracle/tlsan_oracle.py::forward)
 *   score(b, g) = b_g                                               bias               column 0
 *               + sum_c  u_emb[b,c] w_g[c]                          user               column 1
 *               + sum_c  a1[b,0,c] k0[c] w_g[c]                     bridge offset      column 2
 *               + sum_l sum_c' a0[b,l,c'] h[b,l,c'] v_bg[c']        long-term position l   columns 3 .. 3 + Ls - 1
 *               + sum_j sum_c  a1[b,1+j,c] h_new[b,j,c] w_g[c]      session position j     columns 3 + Ls .. R - 1
 *   w_g = item_emb[g] || cate_emb[item_cate[g]],  v_bg = K (a1[b,0,:] o w_g),  h[b,l,:] = e_long[b,l,:] gamma usert[u_b,l] hist_t[b,l],
 *   R = 3 + Ls + Sn.
 * items [B, Kc]: the ids to explain, typically a row's recommendation list; a negative id is padding; an id >= item_count is
 *   TLSAN_E_BADARG before any launch (the call copies `items` to the host for that check and waits for `stream`; it
 *   cannot be captured into a graph).  b->i, b->j and b->y are not read.
 * parts [B, Kc, R] fp32, or NULL.  A position at or past sl[b] (long-term) or sl_new[b] (session) is exactly 0.0f, decided by
 *   the lengths and not by the attention value (a row with sl[b] == 0 has att0 of 0.1 or 0, see tlsan_forward_att: its
 *   long-term columns are 0 either way); every column of a padding item is 0.0f.
 * top_src, top_item [B, Kc, r] int32 and top_val [B, Kc, r] fp32, 1 <= r <= 16, or NULL together: the r strongest history
 *   sources of each (row, item), selected in the same launch.  Columns 0 .. 2 never compete.
 *   by     TLSAN_EXPLAIN_BY_POSITION: every valid position is a source (src = its column, item = the id it holds);
 *          TLSAN_EXPLAIN_BY_ITEM: the valid positions of a row that hold the same item id, in the long window or the
 *          session, are ONE source: its value is the fp32 sum of its positions' parts in ascending column order (one
 *          rounding per addition), its src the lowest of its columns.
 *   order  TLSAN_EXPLAIN_POSITIVE: larger value first;  TLSAN_EXPLAIN_ABS: larger magnitude first, the value keeps its sign.
 *   Equal keys (+0.0 == -0.0) go to the lower src; a NaN comes after every number.  A (row, item) with fewer than r
 *   sources, and every padding item, ends in src = item = -1, val = 0.
 *   The selection runs over the fp32 parts the call writes (or would write): with parts == NULL the same top_* come back bit
 *   for bit, and no [B, Kc, R] array is allocated or written anywhere -- a tile's parts live in LDS.
 * Arithmetic: fp32 throughout; bf16 tables are widened exactly; the K product runs on v_mfma_f32_16x16x4_f32.
 *   p->matrix_dtype is not looked at: with bf16 matrix products the parts decompose the fp32 model's score for the given
 *   attention weights, not the bf16 logit.
 * One launch: a workgroup takes one row and a tile of up to 64 items (LDS holds the tile's w and v rows), so any Kc >= 1.
 * All six (d, heads) pairs, Ls <= 96, Ls + Sn <= 192 (the longest window and session the training step takes;
 * TLSAN_E_UNSUPPORTED beyond: grouping a row's positions by item and ranking an item's sources compare every position
 * with every other, so the cost is quadratic in Ls + Sn).  Row strides and p->scale are honoured as in tlsan_score_candidates.  ws is not
 * used and may be NULL.  Refusals (NULL pointers, B or Kc < 1, B * Kc * R >= 2^31, r outside 1..16 with top_*, an unknown by
 * or order, nothing asked for) come before any launch.  An addition: nothing else in the ABI changed (TLSAN_ABI_VERSION
 * stays 15). */
#define TLSAN_EXPLAIN_BY_POSITION 0
#define TLSAN_EXPLAIN_BY_ITEM 1
#define TLSAN_EXPLAIN_POSITIVE 0
#define TLSAN_EXPLAIN_ABS 1
#define TLSAN_EXPLAIN_RMAX 16
int tlsan_explain(const tlsan_dims* dims, const tlsan_params* p, const tlsan_batch* b, const float* att0, const float* att1,
                  const int32_t* items, int32_t Kc, int32_t r, int32_t by, int32_t order, float* parts, int32_t* top_src,
                  int32_t* top_item, float* top_val, void* ws, size_t ws_bytes, void* stream);

/* Boosted lists: tlsan_eval_topk_scoped and tlsan_eval_topk_lists with a per-item score adjustment applied INSIDE the
 * selection, where a score meets its row's threshold ("promote these items", "bury those", "pay this much for novelty").
 * An item just outside the unboosted list that the boost lifts in is found; a caller who adjusts the returned list
 * afterwards can only reorder its prefix.  Both take the unboosted call's arguments, unchanged in meaning, and two more:
 *   boost: fp32, one value per GLOBAL item id.  The caller guarantees that it covers every global id the id mapping can
 *     produce, 0 .. (item_count - 1) * id_mul + id_add: it is read at n * id_mul + id_add for the local items n the call
 *     scores (in the item-sharded form every rank passes the same, replicated vector).  It is not checked.
 *   row_weight [B] fp32, or NULL: a per-row factor on the boost.
 * With s(b, g) the model's score of row b and the item of global id g, bit for bit what the unboosted call and
 * tlsan_score_candidates return, the adjusted score is
 *     s'(b, g) = fl(s(b, g) + t),   t = boost[g] without row weights, t = fl(row_weight[b] * boost[g]) with them,
 * in fp32 with separate roundings (no fused multiply-add).  Selection, the thresholds, the merge of slices and the order
 * all act on s' by tlsan_eval_topk's rules: higher first, equal s' -> lower global id, +0.0 == -0.0 (returned as +0.0),
 * NaN after everything else.  The scores returned are s'; tlsan_score_candidates on the returned ids gives the raw ones.
 *   boost[g] = -inf gives s' = -inf, a valid score that ranks after every finite one: it is NOT an exclusion (the item
 *     still appears when the row has fewer than K finite candidates).  The exclusion lists, sub and the index remove items.
 *   IEEE rules decide the rest: a NaN boost, or 0 * inf from a zero weight, gives NaN, which ranks last.
 *   A boost of all +0.0 returns exactly the ids and score bits of the unboosted call.
 *   A row's result depends on its own inputs only: not on B, the other rows, the launch geometry or the number of ranks.
 * Neither call changes the parameters, P or any state.  Workspaces: the unboosted calls' (tlsan_scope_workspace_bytes,
 * tlsan_lists_workspace_bytes).  Everything the unboosted call refuses is refused with the same code, before any launch,
 * with this function's name in tlsan_last_error; boost NULL is TLSAN_E_BADARG (the unboosted call exists for that).
 * tlsan_similar_topk*, tlsan_dense_topk and the shortlist index take no boost.  The two functions are additions: nothing
 * else in the ABI changed (TLSAN_ABI_VERSION stays 15). */
int tlsan_eval_topk_scoped_boost(const tlsan_dims* dims, const tlsan_params* p, const float* u_t, int32_t B, int32_t K,
                                 const int32_t* excl_off, const int32_t* excl_ids, const int32_t* sub, int32_t nsub,
                                 const int32_t* row_cate, int32_t id_mul, int32_t id_add, int32_t* ids, float* scores,
                                 void* ws, size_t ws_bytes, void* stream, const float* boost, const float* row_weight);
int tlsan_eval_topk_lists_boost(const tlsan_dims* dims, const tlsan_params* p, const float* u_t, int32_t B, int32_t K,
                                const int32_t* excl_off, const int32_t* excl_ids, const int32_t* list_off,
                                const int32_t* list_items, int32_t nlists, int32_t max_list, const int32_t* row_lists,
                                int32_t P, int32_t id_mul, int32_t id_add, int32_t* ids, float* scores, void* ws,
                                size_t ws_bytes, void* stream, const float* boost, const float* row_weight);

/* Clustered item index: the partition the indexed lists take, LEARNED from the item vectors (k-means over what
 * tlsan_item_vectors writes), and the choice of the lists a query probes.  The three calls take dense fp32 matrices with
 * d = 64, 128 or 256 (16-byte aligned rows), read no table and change no parameter or state; C is the number of
 * centroids, 1 <= C <= 16384.
 *   tlsan_cluster_assign: assign[n] = the centroid nearest to row n of x [N, d] in Euclidean distance, found as the argmax
 *     over j of fl(x_n . c_j) - h_j, h_j = fl(|c_j|^2 / 2) (summed in double), the product on the evaluation scorers' fp32
 *     MFMA chains; equal values -> the lower j; a row whose best value is NaN (or that has none above -inf) -> 0.
 *     dist[n] (dist may be NULL) = max(|x_n|^2 - 2 best_n, 0), the norm summed in double: the row's term of the k-means
 *     objective.  A row's result depends on that row and on cent only: not on N, the other rows or the launch geometry.
 *     Workspace: C floats (tlsan_cluster_workspace_bytes).
 *   tlsan_cluster_means: cent[j] = the mean of the rows x[order[p]], seg_off[j] <= p < seg_off[j + 1] (x [N, d], order [N],
 *     seg_off [C + 1]), summed in double in the order given and rounded once.  An empty segment leaves cent[j] as it is; a
 *     position or a row outside [0, N) is passed over.  No atomics: the result is a function of the inputs, bit for bit.
 *   tlsan_cluster_probe: row_lists[b, 0 .. P) = the P lists of highest s_j = fl(fl((q_b . c_j) * scale_j) + bias_j) (two
 *     roundings, as a score of tlsan_eval_topk; scale NULL: 1, bias NULL: 0) for q [B, d], 1 <= P <= 64, in
 *     tlsan_eval_topk's order: higher first, equal -> lower list, NaN last.  With list_off [C + 1] given, a list with
 *     list_off[j + 1] <= list_off[j] is passed over.  Slots left over (C < P, too few lists with items) hold -1.  A
 *     row's lists depend on that row only.  Workspace: B * P floats.
 *   tlsan_cluster_workspace_bytes(B, C, P): enough for tlsan_cluster_assign with C centroids and for tlsan_cluster_probe of
 *     B rows and P probes (B or P 0: the assignment alone); 0, with tlsan_last_error set, on a refusal.
 * Refused before any launch, with the function's name in tlsan_last_error: a NULL pointer among the required ones, N or B
 * < 1 (N > 2^30, B > 2^24), C outside 1..16384, P outside 1..64 (TLSAN_E_BADARG); d not 64 / 128 / 256
 * (TLSAN_E_UNSUPPORTED); a workspace that is NULL or too small (TLSAN_E_WORKSPACE).  The four functions are additions:
 * nothing else in the ABI changed (TLSAN_ABI_VERSION stays 15). */
size_t tlsan_cluster_workspace_bytes(int32_t B, int32_t C, int32_t P);
int tlsan_cluster_assign(const float* x, int32_t N, int32_t d, const float* cent, int32_t C, int32_t* assign, float* dist,
                         void* ws, size_t ws_bytes, void* stream);
int tlsan_cluster_means(const float* x, int32_t N, const int32_t* order, const int32_t* seg_off, int32_t C, int32_t d,
                        float* cent, void* stream);
int tlsan_cluster_probe(const float* q, int32_t B, int32_t d, const float* cent, const float* scale, const float* bias,
                        const int32_t* list_off, int32_t C, int32_t P, int32_t* row_lists, void* ws, size_t ws_bytes,
                        void* stream);

/* Dense top-K: for each query vector q_i (q [Q, d], d = 64, 128 or 256, 16-byte aligned rows) the K rows of a dense fp32
 * matrix x [N, d] of highest
 *     score(i, n) = fl(fl(acc(q_i, x_n) * q_scale[i]) + q_bias[i])       (q_scale NULL: 1, q_bias NULL: 0; device vectors [Q])
 * selected inside the scoring kernel: the [Q, N] matrix is never materialised, no table is read and no parameter or
 * state changes.  acc is the fp32 MFMA chain of tlsan_eval_topk's tiles with the query in u_t's place; the products
 * commute and the chain's k-order is the same, so with q_i an item's stored vector (tlsan_item_vectors), x_n a row's u_t,
 * q_scale the table scale and q_bias the item's item_b, score(i, n) is tlsan_eval_topk's / tlsan_score_candidates' score
 * of that (row, item) pair bit for bit: the audience of an item -- a user appears in it with exactly the score the item
 * has in that user's list.  The global id of matrix row n is id_add + n (a caller that holds rows [row0, row0 + N) of a
 * larger matrix passes row0 and merges the holders' lists with tlsan_topk_merge).  ids / scores [Q, K] in
 * tlsan_eval_topk's order: higher score first, equal scores -> lower global row id, +0 == -0, NaN last; a query with
 * fewer than K eligible rows ends in -1 / -inf.  excl_off [Q + 1] / excl_ids (both or neither): per-query global row ids,
 * ascending, never selected; listed ids outside [id_add, id_add + N) match no row.
 *   tlsan_dense_topk_workspace_bytes(Q, N, K): the room the slices' lists take, never less for a larger Q, N or K; 0, with
 *     tlsan_last_error set, on sizes the call refuses.
 * Refused before any launch, with the function's name in tlsan_last_error: a NULL q, x, ids or scores, excl_off without
 * excl_ids or the reverse, Q < 1 (Q > 2^24), N < 1 (N > 2^30), id_add < 0 or id_add + N past int32, K outside 1..256
 * (TLSAN_E_BADARG); d not 64 / 128 / 256 (TLSAN_E_UNSUPPORTED); a workspace that is NULL or too small
 * (TLSAN_E_WORKSPACE).  The two functions are additions: nothing else in the ABI changed (TLSAN_ABI_VERSION stays 15). */
size_t tlsan_dense_topk_workspace_bytes(int32_t Q, int32_t N, int32_t K);
int tlsan_dense_topk(const float* q, int32_t Q, int32_t d, const float* x, int32_t N, const float* q_scale, const float* q_bias,
                     const int32_t* excl_off, const int32_t* excl_ids, int32_t id_add, int32_t K, int32_t* ids, float* scores,
                     void* ws, size_t ws_bytes, void* stream);

/* List cursors: tlsan_eval_topk_scoped(_boost), tlsan_eval_topk_lists(_boost) and tlsan_dense_topk continued behind a
 * position of their own ranking, so that pages of K entries tile the exact list at any depth (K itself stays 1..256) for
 * one scan per page; nothing of the earlier pages is kept but one (id, score) pair per row.  The three calls take their
 * twin's arguments, unchanged in meaning, and two more: after_ids [B] int32 and after_scores [B] fp32 (per query, [Q], in
 * global row ids id_add + n, for the dense call).  With key(s, g) the 64-bit order of every list call (higher score first,
 * equal scores -> lower global id, +0.0 == -0.0, NaN after everything else; larger key = earlier) and s'(b, g) the score
 * the call would return for the pair (the model's, or the boosted one):
 *   after_ids[b] >= 0: row b may select item g only when key(s'(b, g), g) < key(after_scores[b], after_ids[b]).  Everything
 *     else about the call is unchanged -- eligibility (exclusion lists, sub, row_cate, the lists), order, padding with
 *     -1 / -inf, the score bits -- so the page is the K best of what the same call without a cursor ranks strictly behind
 *     the cursor.  The cursor is a position in the order, not an item: it need not be in the table, in the scope or
 *     eligible, and its zero's sign and NaN payload do not matter (the key drops both).
 *   after_ids[b] == TLSAN_AFTER_START (-2): no cursor; the row is the twin's, ids and bits.
 *   any other negative id (in particular -1, what the last entry of a short row holds): the row is exhausted; its page is
 *     all -1 / -inf.
 * So with the cursor of a page its last column (ids[:, K - 1], scores[:, K - 1]), pages 1 .. P concatenated are the first
 * P * K entries of the exact ranking; the page after a short page is empty and stays empty; rows of one call may sit at
 * different depths; and a row's page depends on its own inputs only, not on B, the other rows, the launch geometry or the
 * number of ranks (in the item-sharded form every rank applies the same cursor, in global ids; tlsan_topk_merge is
 * unchanged).  Pages tile only while the parameters, the boost, the scope and the exclusions stay the same: a cursor is a
 * snapshot, and nothing detects a change.
 * boost may be NULL here (no adjustment: t = 0, the unboosted score bits); row_weight may be NULL (1) and needs boost.
 * Workspaces: the twins' (tlsan_scope_workspace_bytes, tlsan_lists_workspace_bytes, tlsan_dense_topk_workspace_bytes).
 * Everything the twin refuses is refused with the same code, before any launch, with this function's name in
 * tlsan_last_error; a NULL after_ids or after_scores, and row_weight without boost, are TLSAN_E_BADARG.
 * tlsan_eval_topk itself, tlsan_similar_topk*, tlsan_eval_shelves, the shortlist index and tlsan_rerank take no cursor.
 * The three functions and the constant are additions: nothing else in the ABI changed (TLSAN_ABI_VERSION stays 15). */
#define TLSAN_AFTER_START (-2)
int tlsan_eval_topk_scoped_after(const tlsan_dims* dims, const tlsan_params* p, const float* u_t, int32_t B, int32_t K,
                                 const int32_t* excl_off, const int32_t* excl_ids, const int32_t* sub, int32_t nsub,
                                 const int32_t* row_cate, int32_t id_mul, int32_t id_add, int32_t* ids, float* scores,
                                 void* ws, size_t ws_bytes, void* stream, const float* boost, const float* row_weight,
                                 const int32_t* after_ids, const float* after_scores);
int tlsan_eval_topk_lists_after(const tlsan_dims* dims, const tlsan_params* p, const float* u_t, int32_t B, int32_t K,
                                const int32_t* excl_off, const int32_t* excl_ids, const int32_t* list_off,
                                const int32_t* list_items, int32_t nlists, int32_t max_list, const int32_t* row_lists,
                                int32_t P, int32_t id_mul, int32_t id_add, int32_t* ids, float* scores, void* ws,
                                size_t ws_bytes, void* stream, const float* boost, const float* row_weight,
                                const int32_t* after_ids, const float* after_scores);
int tlsan_dense_topk_after(const float* q, int32_t Q, int32_t d, const float* x, int32_t N, const float* q_scale,
                           const float* q_bias, const int32_t* excl_off, const int32_t* excl_ids, int32_t id_add, int32_t K,
                           int32_t* ids, float* scores, void* ws, size_t ws_bytes, void* stream, const int32_t* after_ids,
                           const float* after_scores);

/* bf16 shortlist index: the exact top K over the whole table in two stages, with a per-row CERTIFICATE that the cheap
 * first stage lost nothing.  With w_n = [item_emb[n] || cate_emb[item_cate[n]]] as stored (d columns, the table scale P
 * not folded) and row b's u_t:
 *   tlsan_shortlist_build: the snapshot.  vec [item_count, d] bf16 (uint16 patterns) = w_n rounded to nearest even -- a
 *     bf16 table's values are copied, not rounded again; *wmax (a device float) = max_n ||w_n||_2 of the STORED fp32
 *     values, every norm summed in fp32 in one fixed order and the maximum taken on bit patterns: the same table gives
 *     the same bits, whatever the launch.  Non-finite (+inf) when any element is, or when a sum of squares overflows.
 *   tlsan_shortlist_topk (stage 1): ids / approx [B, N], 16 <= N <= 256: the N items of highest APPROXIMATE score
 *       a~(b, n) = fl(fl(acc~ * P) + item_b[n * ld_itemb]),
 *     acc~ the fp32 accumulation by v_mfma_f32_16x16x32_bf16 of bf16(u_t[b]) . vec[n] (u_t rounded to nearest even; scale
 *     NULL: P = 1), in tlsan_eval_topk's order on (a~, global id); the exclusion lists and id_mul / id_add are
 *     tlsan_eval_topk's.  Rows with fewer than N eligible items end in id -1, approx -inf.  A row's result depends on that
 *     row only.  Workspace: tlsan_shortlist_workspace_bytes(I, B, d, N) (never 0 for sizes the call accepts).
 *   tlsan_shortlist_select (stage 2): from sl_ids / sl_approx [B, N] (stage 1's) and sl_exact [B, N], the shortlist's scores
 *     by tlsan_score_candidates -- the exact path's bits -- ids / scores [B, K], 1 <= K < N: the K entries of highest exact
 *     score in tlsan_eval_topk's order (short rows end in -1 / -inf), and certified [B] int32.  With s_K the K-th best exact
 *     score of the shortlist, a~_N the approximate score of its N-th entry and
 *       eps_b = c |P| ||u_t[b]||_2 wmax + 2^-20 (|s_K| + |a~_N|),   c = 2^-7 + 2^-11
 *     (the norm in fp32 from the fp32 u_t, the rest in double), certified[b] = 1 when the shortlist holds fewer than N
 *     valid entries (every eligible item is in it), or when s_K, a~_N and eps_b are finite and s_K > a~_N + eps_b, strictly;
 *     else 0.  certified[b] = 1 means ids / scores [b] ARE tlsan_eval_topk's row, ids and score bits (DESIGN.md section 7
 *     has the proof); a row with 0 is to be served by tlsan_eval_topk.
 * vec is 16-byte aligned (both kernels move it 16 bytes at a time); its rows are d bf16 values, densely packed.
 * No call changes the parameters, P or any state.  Refused before any launch, with the function's name in
 * tlsan_last_error: a NULL pointer among the required ones, N outside 16..256, K outside 1..N-1, I outside 1..2^30, B outside
 * 1..2^24, excl_off without excl_ids or the reverse, ld_itemb < 1, an id mapping that leaves int32, d_item / d_cate that are
 * no multiples of 4 adding up to d, an unknown table_dtype (TLSAN_E_BADARG); d not 64 / 128 / 256, or -- stage 1 and its
 * workspace call -- B * slices * N at or above 2^31, slices the item slices of the launch (TLSAN_E_UNSUPPORTED); a
 * workspace that is NULL or too small (TLSAN_E_WORKSPACE).  The four functions are additions: nothing else in the ABI
 * changed (TLSAN_ABI_VERSION stays 15). */
int tlsan_shortlist_build(const tlsan_dims* dims, const tlsan_params* p, uint16_t* vec, float* wmax, void* stream);
size_t tlsan_shortlist_workspace_bytes(int32_t I, int32_t B, int32_t d, int32_t N);
int tlsan_shortlist_topk(const uint16_t* vec, int32_t I, int32_t d, const float* u_t, int32_t B, const float* scale,
                         const float* item_b, int32_t ld_itemb, int32_t N, const int32_t* excl_off, const int32_t* excl_ids,
                         int32_t id_mul, int32_t id_add, int32_t* ids, float* approx, void* ws, size_t ws_bytes, void* stream);
int tlsan_shortlist_select(const int32_t* sl_ids, const float* sl_exact, const float* sl_approx, const float* u_t,
                           const float* scale, const float* wmax, int32_t B, int32_t d, int32_t N, int32_t K, int32_t* ids,
                           float* scores, int32_t* certified, void* stream);

/* Diversified lists: the second stage behind tlsan_eval_topk. From each row's POOL of N entries (1 <= K <= N <= 256, in
 * tlsan_eval_topk's order: higher score first, ties -> lower global id) pick K by greedy maximal marginal relevance
 * under a per-category cap.  Pool entry j of a row has a global id g_j and the model score s_j (pool_ids, pool_scores
 * [B, N]), and, at flattened position b * N + j, its stored vector w_j (vec [B * N, d], d = 64, 128 or 256), inv_j (inv
 * [B * N]) -- both what tlsan_item_vectors wrote for the flattened pool ids, so an id -1 has zeros -- and its category
 * c_j (cate [B * N]).  The call reads no table: one form serves a whole table and a sharded one, with the same bits.
 *   Valid entries: g_j >= 0 and s_j finite.  The others are never selected.
 *   Relevance: r_j = (s_j - s_lo) / (s_hi - s_lo), s_hi / s_lo the scores of the row's first / last valid entry;
 *     r_j = 0 for every j when s_hi == s_lo.
 *   Similarity: cos(i, j) = (w_i . w_j) * (inv_i * inv_j) in fp32, the sum in one fixed order that depends on d and
 *     the lane only; a zero row has inv 0 and so cos 0; the table scale P cancels, as in TLSAN_SIM_COSINE.
 *   Greedy selection, t = 1 .. K, with diversity theta in [0, 1] and per_category m >= 0 (0: no cap):
 *     eligible entries are valid, not yet selected and (m > 0) share their category with fewer than m selected entries;
 *     the value of j is (1 - theta) r_j for t = 1, afterwards (1 - theta) r_j - theta * max over the selected i of
 *     cos(i, j); the eligible entry of largest value is picked, equal values -> lower pool position; when no entry is
 *     eligible the row ends there and the remaining outputs are id -1, score -inf.
 *     A value that is NaN (a vector holding inf or NaN) counts as -inf.
 *   Output: ids [B, K], scores [B, K] in selection order; the scores are the pool's own s_j, bit for bit.
 *   theta = 0, m = 0 returns the valid entries of the pool in their order (the first K entries unchanged when they
 *   are valid).  theta = 0, m > 0: a row that comes back with K valid entries is the capped greedy ranking over ALL
 *   eligible items of the table, because the pool is the exact score-order prefix; a short row means the pool was too
 *   small.  With theta = 0 no product is formed: the selection is integer logic on the order of the scores.
 *   A row's result depends on its own pool only: not on B, the other rows, the launch geometry or the number of ranks.
 * Refused before any launch, with the function's name in tlsan_last_error: NULL pointers, N outside 1..256, K outside
 * 1..N, theta outside [0, 1] or NaN, m < 0, B < 1 or B * N >= 2^31 (TLSAN_E_BADARG), d not 64 / 128 / 256
 * (TLSAN_E_UNSUPPORTED).  An addition: nothing else in the ABI changed (TLSAN_ABI_VERSION stays 14). */
int tlsan_rerank(const int32_t* pool_ids, const float* pool_scores, const float* vec, const float* inv,
                 const int32_t* cate, int32_t B, int32_t N, int32_t d, int32_t K, float diversity, int32_t per_category,
                 int32_t* ids, float* scores, void* stream);

/* List metrics: what a recommendation list looks like beside its accuracy.  A row is a list of K entries (1 <= K <= 256):
 * ids [B, K] global item ids, -1 = no entry, ANYWHERE in the row (a caller-given list need not be a tlsan_eval_topk list);
 * at flattened position b * K + j the entry's stored vector (vec [B * K, d], d = 64, 128 or 256) and inverse norm (inv
 * [B * K]) -- both what tlsan_item_vectors wrote for the flattened ids, so an id -1 has zeros and a zero row has inv 0 --
 * and its category (cate [B * K]).  Like tlsan_rerank the call reads no table: one form serves a whole table and a
 * sharded one, with the same bits.  Per row, over its VALID entries (id >= 0) in position order:
 *   n_valid [B]     their number n.
 *   pair_cos [B]    the sum over valid i < j of cos(i, j) = fl((w_i . w_j) * fl(inv_i * inv_j)), tlsan_rerank's cosine (the
 *     fp32 dot in one fixed order that depends on d and the lane only; a zero vector has cosine 0 against everything),
 *     accumulated in double in ONE order: c_j = ((0 + cos(i0, j)) + cos(i1, j)) + ... over the valid i < j ascending, then
 *     pair_cos = ((0 + c_0) + c_1) + ... over j ascending (c_j = 0 for an entry that is not valid).  Exactly 0.0 for n < 2.
 *     The intra-list diversity is ILD = 1 - pair_cos / (n (n - 1) / 2), formed by the caller (NaN for n < 2, not clamped).
 *   n_cate [B]      distinct categories among the valid entries.
 *   max_cate [B]    the largest number of valid entries that share one category, 0 for an empty row: a list made with
 *     tlsan_rerank's per_category = m shows max_cate <= m.
 *   hit_pos [B]     the first position j (a position in the list, holes counted) with a valid ids[b, j] == labels[b] where
 *     labels[b] >= 0; -1 when the label is absent or negative, or labels is NULL.
 *   weight_sum [B]  ((0 + weight[b K + j0]) + weight[b K + j1]) + ... in double over the valid j ascending; 0 when weight
 *     is NULL.  The novelty hook: the caller passes each entry's self-information.
 *   exposure [n_items] (nullable)  exposure[g] += 1 for every valid entry with g < n_items (integer atomics: the result
 *     does not depend on the order); ids >= n_items are skipped.  The call adds to the array and never clears it.
 * A row's outputs depend on its own list only: not on B, the other rows, the launch geometry or a second run; there are
 * no floating-point atomics.
 * Refused before any launch, with the function's name in tlsan_last_error: B < 1 or B * K >= 2^31, K outside 1..256,
 * exposure given with n_items < 1, NULL among ids / vec / inv / cate or the six per-row outputs ("tlsan_list_metrics:
 * NULL argument") (TLSAN_E_BADARG), d not 64 / 128 / 256 (TLSAN_E_UNSUPPORTED).  An addition: nothing else in the ABI
 * changed (TLSAN_ABI_VERSION stays 14). */
int tlsan_list_metrics(const int32_t* ids, const float* vec, const float* inv, const int32_t* cate,
                       const int32_t* labels, const float* weight, int32_t B, int32_t K, int32_t d, int32_t* n_valid,
                       double* pair_cos, int32_t* n_cate, int32_t* max_cate, int32_t* hit_pos, double* weight_sum,
                       uint32_t* exposure, int32_t n_items, void* stream);

/* Scores of caller-given candidates (a re-ranking of a retrieval stage's items, or a sampled evaluation):
 *   scores[b, c] = u_t[b] . [item_emb || cate_emb[item_cate]][g] + item_b[g],  g = cand[b, c] (global id),
 * for u_t [B, d], cand [B, C] int32, scores [B, C] float32.  Each score equals tlsan_eval_label_scores' for the
 * same (row, item) bit for bit -- and so a tlsan_eval_topk list entry's -- with lazy L2 (P != 1) and bf16 tables.
 *   Whole table (id_mul == 1, id_add == 0): ids outside 0 .. item_count-1 (the padding -1 among them) score -inf.
 *   Item-sharded form: local item n is global id n * id_mul + id_add, as in tlsan_eval_counts_shard; a candidate
 *     this table does not hold is skipped and its score left untouched (each rank scores its own ids).
 * The result does not depend on B, C, on the other rows of the launch or on the launch geometry.  B, C >= 1. */
int tlsan_score_candidates(const tlsan_dims* dims, const tlsan_params* p, const float* u_t, int32_t B, int32_t C,
                           const int32_t* cand, int32_t id_mul, int32_t id_add, float* scores, void* stream);
/* ranks[b] = how many candidates c >= 1 of row b come ahead of candidate 0 (the label) in tf.nn.top_k's order, as
 * tlsan_eval_topk orders: higher score first, equal scores -> lower global id first; +0.0 == -0.0; a NaN score
 * comes after every other score.  Candidates with a negative id (padding) and repeats of candidate 0's id are not
 * counted.  With every other item as a candidate this is tlsan_eval_ranks' rank.  cand, scores [B, C]. */
int tlsan_candidate_ranks(const int32_t* cand, const float* scores, int32_t B, int32_t C, int32_t* ranks, void* stream);
/* N distinct negatives per row, 1 <= N <= 1024, reproducible from their definition alone.  Row b is the global row
 * row = row0 + b; with splitmix64 the standard finaliser (uint64 arithmetic, wrapping), draw t = 0, 1, 2, ... of the
 * row is the item  ((key >> 32) * item_count) >> 32,  key = splitmix64(splitmix64(seed ^ row) ^ t).
 * out[b] holds the first N distinct items of that sequence that are eligible -- not labels[b], not in the row's
 * exclusion list (excl_off [B + 1] / excl_ids, both NULL for none: as tlsan_eval_topk's) -- among the first 64 N
 * draws; slots left unfilled hold -1.  The result depends on (seed, row, label, exclusion list, item_count, N) only:
 * not on B, the chunking of the rows, the launch geometry or the number of ranks.  out [B, N] int32. */
int tlsan_sample_negatives(int32_t item_count, const int32_t* labels, int32_t B, int32_t N, uint64_t seed, int64_t row0,
                           const int32_t* excl_off, const int32_t* excl_ids, int32_t* out, void* stream);

/* Deterministic scatter-apply on one row table (the owner-side half of the multi-GPU step, and
 * the stand-alone form of the embedding update of model.py:198-205):
 *   for every row r < nrows:  g = gscale * sum_{k: dest[k]==r} grows[k] (+ reg * W[r] on the
 *   first reg_cols columns);   W[r] -= (*step_dev) * g
 * Rows without contributions still decay (dense L2, as the reference).  The sum is exact
 * (order independent) -> bitwise reproducible.  width % 4 == 0, width <= 192.
 * sumsq_out (nullable, device double) receives sum over the first reg_cols columns of W_new^2.
 * step_dev is a DEVICE float (lr * clip coefficient) so no host sync is needed. */
size_t tlsan_rows_apply_workspace(int32_t nrows, int32_t n);
int tlsan_rows_apply(float* W, int32_t ld, int32_t nrows, int32_t width, int32_t reg_cols,
                     const float* grows, int32_t ldg, const int32_t* dest, int32_t n,
                     float gscale, const float* step_dev, float reg, double* sumsq_out,
                     void* ws, size_t ws_bytes, void* stream);

/* ---- device side of the row-sharded multi-GPU step (tlsan_amd/dist.py; no reference counterpart:
 * the reference is single-GPU, train.py:53,146).  Key space: G owners x R rows, key = owner*R + row.
 *
 * tlsan_route_plan: distinct rows a batch touches, grouped by owner (= all-to-all send order):
 *   keys [n_keys] (duplicates fine) -> rank[G*R] compact index of every key, uniq[<=n_keys]
 *   distinct keys ascending, n_uniq[1], cate_c[n_uniq] = cate_by_key[uniq], comp[n_keys] = rank[keys],
 *   sendbuf [G][1 + cap] = per owner {count, row numbers inside the owner's shard ...}: the payload of
 *   ONE equal-split all-to-all.  cap must be the same on every rank (the exchange is equal-split);
 *   when it is smaller than min(R, n_keys), what this batch may need, no rows are written and every
 *   count is -min(R, n_keys): all ranks then see the same negative counts after the exchange, agree on a
 *   larger cap and repeat the plan.  cate_c entries [n_uniq, cate_pad) are set
 *   to -1 (a compact table padded to a fixed row count).  flags[G*R] is scratch that must be zero
 *   on entry and is zero again on exit.  counts_out (optional, [G]): the per-owner counts once more,
 *   written by the kernel -- pass device-visible pinned host memory to have the exchange sizes on
 *   the host without a copy. */
int tlsan_route_plan(const int32_t* keys, int32_t n_keys, int32_t R, int32_t G, const int32_t* cate_by_key,
                     int32_t* flags, int32_t* rank, int32_t* uniq, int32_t* n_uniq, int32_t* sendbuf, int32_t cap,
                     int32_t* cate_c, int32_t cate_pad, int32_t* comp, int32_t* counts_out, void* stream);

/* tlsan_shard_gather: owner side of the row fetch.  recvbuf [G][1 + cap] as received from the G
 * ranks; n_recv = sum of the counts (host value).  rows_out [n_recv, W] = the requested rows of
 * shard [R, ld] in source-rank order (the all-to-all send order), recv_rows [n_recv] = their row
 * numbers (input of tlsan_shard_apply). */
int tlsan_shard_gather(const float* shard, int32_t ld, int32_t R, int32_t W, const int32_t* recvbuf, int32_t cap,
                       int32_t G, int32_t n_recv, float* rows_out, int32_t* recv_rows, void* stream);

/* tlsan_shard_summary: after the all-reduce (sum over G ranks) of
 *   flat = [dense grads n_dense | cate grads n_cate | mean BCE | per-use row squares | table squares | pad]:
 * global norm (tf18 rule), clip coefficient (model.py:201), loss (model.py:164-172), the device
 * step size lr*coef (step_dev[0]; step_dev[1] = coef), and the SGD update of the replicated dense
 * parameters (+ K^T copy). */
int tlsan_shard_summary(const float* flat, int32_t n_dense, int32_t n_cate, int32_t G, float lr, float reg, float clip,
                        const double* S_cate, float* dense, float* dense_KT, const tlsan_dims* dims,
                        float* step_dev, float* loss_out, float* gnorm_out, void* stream);

/* The other optimizers (tlsan_optimizer above: same kinds, defaults and arithmetic) on the sharded step:
 * accumulators laid out like what they belong to -- the shard rows [R, ld], cate_emb [C, dc] and the
 * dense parameters (the last two replicated: every rank applies the same update).  kind SGD / NULL =
 * the plain functions.  item_b (column reg_item of an item row) is touched where a gradient arrived
 * (sparse RMSProp / Adadelta) or everywhere (Adam), as on one GPU. */
typedef struct {
  int32_t kind, step;
  float beta1, beta2, epsilon;
  float* shard_s1; float* shard_s2;
  float* cate_s1; float* cate_s2;
  float* dense_s1; float* dense_s2;
  /* lazy L2 on the sharded step (kind SGD only; the accumulators may then be NULL): the tables are
   * scale[0] * stored, one scale that every rank advances alike (tlsan_shard_apply_lazy commits it);
   * step_dev then has 4 floats: {lr coef, coef, lr coef / P_new, P_new}. */
  float* scale;
} tlsan_shard_optimizer;
int tlsan_shard_summary_opt(const float* flat, int32_t n_dense, int32_t n_cate, int32_t G, float lr, float reg, float clip,
                            const double* S_cate, float* dense, float* dense_KT, const tlsan_dims* dims,
                            float* step_dev, float* loss_out, float* gnorm_out, const tlsan_shard_optimizer* opt,
                            void* stream);

/* tlsan_shard_apply: owner-side update of the fused shard table [R, W] (rows [0,cI) items with
 * reg_item regularised columns, rows [cI,R) users with reg_user) from the row gradients received
 * from every rank (vals[n_recv, ldv] for local rows `rows`, concatenated in source-rank order,
 * src_off[G+1] host array of the per-source offsets; rows of one source are distinct), and of the
 * replicated category table from g_cate [C, dc]:  W -= step * (gscale * sum + reg * W) on every
 * row (dense L2, as the reference).  Fixed summation order -> bitwise reproducible.
 * slots: int32 [R*G] device scratch that must be zero on entry and is zero again on exit.
 * sumsq_out[2] (device doubles): sums of squares of the regularised columns of shard / cate_emb
 * after the update; sumsq_f32 (nullable) receives (float)sumsq_out[0].
 * Refused before any launch, with nothing written (these two calls and tlsan_shard_apply_lazy alike): G outside 1..16,
 * W or dc no multiple of 4, W or dc above 256 (the dense forms), a stamp of 0 (the lazy form): TLSAN_E_UNSUPPORTED;
 * src_off that does not run from 0 to n_recv: TLSAN_E_BADARG; ws_bytes below the _workspace value: TLSAN_E_WORKSPACE. */
size_t tlsan_shard_apply_workspace(int32_t R, int32_t C);
int tlsan_shard_apply(float* shard, int32_t ld, int32_t cI, int32_t R, int32_t W, int32_t reg_item, int32_t reg_user,
                      const float* vals, int32_t ldv, const int32_t* rows, int32_t n_recv, const int32_t* src_off,
                      int32_t G, int32_t* slots, float gscale, const float* step_dev, float reg,
                      float* cate_emb, int32_t C, int32_t dc, const float* g_cate,
                      double* sumsq_out, float* sumsq_f32, void* ws, size_t ws_bytes, void* stream);
int tlsan_shard_apply_opt(float* shard, int32_t ld, int32_t cI, int32_t R, int32_t W, int32_t reg_item, int32_t reg_user,
                          const float* vals, int32_t ldv, const int32_t* rows, int32_t n_recv, const int32_t* src_off,
                          int32_t G, int32_t* slots, float gscale, const float* step_dev, float reg,
                          float* cate_emb, int32_t C, int32_t dc, const float* g_cate,
                          double* sumsq_out, float* sumsq_f32, const tlsan_shard_optimizer* opt, float lr,
                          void* ws, size_t ws_bytes, void* stream);

/* tlsan_shard_apply_lazy: the owner-side update in its lazy-L2 form,
 *   W_stored -= (lr coef / P_new) * gscale * sum   for the rows whose gradients arrived (and every row of the
 * replicated category table), item_b (column reg_item of item rows, not regularised, not scaled) -= lr coef * ...
 * -- the same update as tlsan_shard_apply's dense sweep up to fp32 rounding, touching n_recv rows instead
 * of R.  slots64: uint64 [R*G] scratch, any content (entries carry `stamp`, which must differ from step
 * to step and never be 0 for a zero-initialised buffer).  sumsq_out[0] += the change of the stored shard
 * rows' sum of squares (regularised columns), sumsq_out[1] = that of cate_emb (stored values).
 * ws: tlsan_shard_apply_lazy_workspace(n_recv, C) bytes. */
size_t tlsan_shard_apply_lazy_workspace(int32_t n_recv, int32_t C);
int tlsan_shard_apply_lazy(float* shard, int32_t ld, int32_t cI, int32_t R, int32_t W, int32_t reg_item, int32_t reg_user,
                           const float* vals, int32_t ldv, const int32_t* rows, int32_t n_recv, const int32_t* src_off,
                           int32_t G, uint64_t* slots64, uint32_t stamp, float gscale, const float* step_dev,
                           float* cate_emb, int32_t C, int32_t dc, const float* g_cate,
                           double* sumsq_out, float* sumsq_f32, float* scale, void* ws, size_t ws_bytes, void* stream);

/* tlsan_shard_apply_lazy_opt: the owner-side update of lazy Adam / RMSProp / Adadelta -- the dense optimizer's step of
 * tlsan_shard_apply_opt, from the same parameters and accumulators, restricted to the rows the GLOBAL batch (all ranks'
 * batches together) used.  The arguments of tlsan_shard_apply_lazy, plus reg, cate_use, opt and lr.
 *   item / user rows: the rows in `rows` (every received row is a use).  A used row gets, on its live columns,
 *     g = coef * (gscale * sum over the sources in source order, in double + reg * W on the regularised columns)
 *     and the optimizer's step with its two accumulators.  item_b (column reg_item of an item row; reg_item < W) moves where
 *     its summed gradient is not zero, for all three kinds.  Padding columns and rows nobody sent keep W and both
 *     accumulators bit for bit.
 *   category rows: row c is used iff cate_use[c] != 0.  cate_use [C] must hold the same bits on every rank:
 *     tlsan_shard_cate_use(cate_c, n, u_cate, B, C, use) writes this rank's part -- use[c] = 1 for the categories of its
 *     batch (cate_c [n]: the item -> category map of the step's compact table, -1 for the rows that are no items, as
 *     tlsan_route_plan leaves it; u_cate [B]: the batch's), 0 elsewhere -- into C floats that tlsan_amd/dist.py keeps at the
 *     end of the vector the step all-reduces anyway, so cate_use[c] is the number of ranks that used c: exact in fp32.
 *   opt: kind ADAM, RMSPROP or ADADELTA (TLSAN_OPT_LAZY may be OR-ed in; SGD is TLSAN_E_BADARG: tlsan_shard_apply_lazy),
 *     shard_s1/2 and cate_s1/2 given (TLSAN_E_BADARG names the missing one), dense_s1/2 not looked at (the dense weights
 *     move in tlsan_shard_summary_opt, under the dense kind).  opt->scale must be NULL (TLSAN_E_UNSUPPORTED): the update
 *     works on the stored values, the table scale P is 1 and stays 1; a state with P != 1 must be folded first.
 *   step_dev: as tlsan_shard_summary_opt leaves it without a scale ([1] = clip coefficient).
 *   sumsq_out[0] += the change of the shard rows' sum of squares (regularised columns), sumsq_out[1] += that of cate_emb:
 *     both stay the tables' sums while only some rows are written.  sumsq_f32 (nullable) receives (float)sumsq_out[0].
 * W, dc <= 256 and G <= 16 as tlsan_shard_apply (TLSAN_E_UNSUPPORTED).  Fixed summation order, no atomics: bitwise
 * reproducible.  ws: tlsan_shard_apply_lazy_opt_workspace(n_recv, C) bytes.  There is no static-shape form of this call.
 * The three functions are additions: nothing else in the ABI changed (TLSAN_ABI_VERSION stays 14). */
int tlsan_shard_cate_use(const int32_t* cate_c, int32_t n, const int32_t* u_cate, int32_t B, int32_t C, float* use, void* stream);
size_t tlsan_shard_apply_lazy_opt_workspace(int32_t n_recv, int32_t C);
int tlsan_shard_apply_lazy_opt(float* shard, int32_t ld, int32_t cI, int32_t R, int32_t W, int32_t reg_item, int32_t reg_user,
                               const float* vals, int32_t ldv, const int32_t* rows, int32_t n_recv, const int32_t* src_off,
                               int32_t G, uint64_t* slots64, uint32_t stamp, float gscale, const float* step_dev, float reg,
                               float* cate_emb, int32_t C, int32_t dc, const float* g_cate, const float* cate_use,
                               double* sumsq_out, float* sumsq_f32, const tlsan_shard_optimizer* opt, float lr,
                               void* ws, size_t ws_bytes, void* stream);

/* ---- static-shape forms of the sharded step (tlsan_amd/dist.py, ShardedModel(static_rows=True)).
 * Every (source, owner) pair exchanges exactly `cap` row slots in both directions, so no size ever has to reach
 * the host: the ids, the rows and the gradients travel in equal-split all-to-alls of fixed size, every kernel
 * argument is a constant of the shape, and a step can be recorded in a HIP graph.  The step's compact table is
 * numbered by slot: the j-th distinct row of owner g is compact row g * cap + j (at one rank: the plain compact
 * numbering); unused slots are in no category and never referenced.
 *
 * tlsan_route_plan_static: as tlsan_route_plan with that numbering; cate_c has G * cap entries.
 *   counts_out (optional [G]): the TRUE per-owner counts; the headers of sendbuf are clamped to cap.
 *   status [1] (device int32, zero-initialised by the caller): atomicMax of every count that exceeded cap.  A
 *   batch that needs more than cap rows of one owner is truncated -- that step is wrong; the host checks status
 *   when it next synchronises and must report it (cap >= min(R, n_keys) can never overflow).
 * tlsan_shard_gather_static: rows_out [G * cap, W], recv_rows [G * cap] (-1 = empty slot); when slots64 is
 *   given, the lazy apply's slot marks are written here (saves a launch): stamp is a DEVICE uint32 (never 0).
 * tlsan_shard_apply_lazy_static: tlsan_shard_apply_lazy over the G * cap slots (rows[e] < 0: skipped); the
 *   device-side stamp is advanced for the next step: stamps run 1 .. 2^32 - 2, the successor of 2^32 - 2 is 1 (the
 *   numbering tlsan_amd/dist_step.py gives the host-side stamp of tlsan_shard_apply_lazy).  marked != 0: the slot marks
 *   were written by the gather. */
int tlsan_route_plan_static(const int32_t* keys, int32_t n_keys, int32_t R, int32_t G, const int32_t* cate_by_key,
                            int32_t* flags, int32_t* rank, int32_t* uniq, int32_t* n_uniq, int32_t* sendbuf, int32_t cap,
                            int32_t* cate_c, int32_t* comp, int32_t* counts_out, int32_t* status, void* stream);
int tlsan_shard_gather_static(const float* shard, int32_t ld, int32_t R, int32_t W, const int32_t* recvbuf, int32_t cap,
                              int32_t G, float* rows_out, int32_t* recv_rows, uint64_t* slots64, const uint32_t* stamp,
                              void* stream);
/* tlsan_shard_gather_wire_bf16: tlsan_shard_gather_static with bf16 rows on the wire.  Owners keep fp32 rows; slot e
 * of rows_out (pitch bytes per slot, a multiple of 16) receives
 *   [ the first d_emb floats of the row as bf16, round to nearest even | the next `tail` floats as fp32 | pad ]
 * -- for the fused [item_emb | item_b] / [user_emb | usert_emb] rows of tlsan_amd/dist.py: tail = max(1, Ls).  The
 * consumer points its tlsan_params, table_dtype = TLSAN_TABLE_BF16, into the slots: item_emb / user_emb at the slot base
 * with ld = pitch / 2, item_b / usert_emb at base + 2 * d_emb bytes with ld = pitch / 4. */
int tlsan_shard_gather_wire_bf16(const float* shard, int32_t ld, int32_t R, int32_t d_emb, int32_t tail,
                                 const int32_t* recvbuf, int32_t cap, int32_t G, void* rows_out, int32_t pitch,
                                 int32_t* recv_rows, uint64_t* slots64, const uint32_t* stamp, void* stream);
int tlsan_shard_apply_lazy_static(float* shard, int32_t ld, int32_t cI, int32_t R, int32_t W, int32_t reg_item, int32_t reg_user,
                                  const float* vals, int32_t ldv, const int32_t* rows, int32_t cap, int32_t G,
                                  uint64_t* slots64, uint32_t* stamp, int32_t marked, float gscale, const float* step_dev,
                                  float* cate_emb, int32_t C, int32_t dc, const float* g_cate,
                                  double* sumsq_out, float* sumsq_f32, float* scale,
                                  void* ws, size_t ws_bytes, void* stream);

/* ---- the static-shape step in as few host calls as there are collectives (round 4) -------------------------------
 * tlsan_amd/dist.py issued the step as ~15 Python-level calls (ctypes with 10-27 arguments each, torch events, a
 * stream-scoped copy): at one rank the HOST took 100 us per step for 77 us of kernels -- every rank of a multi-GPU run
 * would have been bound by its Python thread.  The two entry points below run the same launches from argument blocks
 * that are built once per (plan slot, batch): one call per segment between two collectives.
 *
 * tlsan_shard_step_static(s, phases, stream): the main stream's launches, `phases` = any contiguous run of
 *   TLSAN_PHASE_GATHER  tlsan_shard_gather_static / _wire_bf16 (s->wire)       -- then the row all-to-all
 *   TLSAN_PHASE_GRADS   tlsan_grads on the compact table                        -- then the all-reduce of s->flat
 *   TLSAN_PHASE_SUMMARY tlsan_shard_summary_opt                                 -- then the gradient all-to-all
 *   TLSAN_PHASE_APPLY   tlsan_shard_apply_lazy_static
 *   (one rank: all four in one call).  `plans` (optional) are issued behind the call's last launch -- they run on their own
 *   streams, and their slots were last used by earlier steps: with s->out.started set (a pinned host word the fused
 *   kernel stores s->out.started_value into when it begins to run; values count up from step to step) the call first
 *   waits, on the HOST, until the word has reached s->plans_after -- "step plans_after has started" = every step before
 *   it is complete -- instead of ordering the side streams behind an event recorded on the main stream (a barrier
 *   packet in the main queue: ~6 us of idle GPU per step).  Without the word the plans carry ev_fork.
 * tlsan_shard_plan_static(p): a batch's routing plan, category index and destination index on p->stream / p->stream2
 *   (tlsan_route_plan_static -- its closing kernel stores an overflow count into the pinned word --, tlsan_state_recategorize, tlsan_batch_index),
 *   ordered by the caller's HIP events (raw hipEvent_t / hipStream_t handles; NULL events are skipped):
 *     stream waits ev_fork; ev_planned recorded behind the route plan; stream2 waits ev_planned, builds the index,
 *     records ev_done1; ev_done0 recorded on stream last when record_done0 != 0 (the caller records it itself when it
 *     puts the id all-to-all there).  stream2 == NULL: the index follows on stream. */
#define TLSAN_PHASE_GATHER 1
#define TLSAN_PHASE_GRADS 2
#define TLSAN_PHASE_SUMMARY 4
#define TLSAN_PHASE_APPLY 8
#define TLSAN_PLAN_ASYNC 256   /* `plans` are issued by the library's launch thread (see tlsan_shard_plans_flush) */
typedef struct {
  const int32_t* keys; int32_t n_keys, R, G; const int32_t* cate_by_key;
  int32_t *flags, *rank, *uniq, *n_uniq, *sendbuf; int32_t cap;
  int32_t *cate_c, *comp, *status;
  int32_t* status_host;                  /* optional PINNED host word: receives the count of an overflowing owner (a system-scope store of the plan's kernel) */
  const tlsan_dims* dims; const tlsan_params* cp; const tlsan_batch* cb; void* state;
  void *stream, *stream2;                /* hipStream_t */
  void *ev_fork, *ev_planned, *ev_done0, *ev_done1;   /* hipEvent_t or NULL */
  int32_t record_done0;
} tlsan_static_plan;
typedef struct {
  /* gather */
  const float* shard; int32_t ld, R, W; const int32_t* recvbuf; int32_t cap, G; void* rows_out; int32_t* recv_rows;
  uint64_t* slots64; uint32_t* stamp;
  int32_t wire, d_emb, tail, pitch;      /* wire != 0: tlsan_shard_gather_wire_bf16(d_emb, tail, pitch) */
  /* grads */
  const tlsan_dims* dims; const tlsan_params* cp; const tlsan_batch* cb; tlsan_hparams hp; tlsan_grads_out go; tlsan_step_out out;
  void* state; void* ws; size_t ws_bytes;
  /* summary */
  float* flat; int32_t n_dense, n_cate; float lr, reg, clip; const double* S_cate; float* dense; float* dense_KT;
  const tlsan_dims* dims_full; float* step_dev; float* loss_out; float* gnorm_out; const tlsan_shard_optimizer* opt;
  /* apply */
  int32_t cI, reg_item, reg_user; const float* vals; int32_t ldv, marked; float gscale; float* cate_emb; int32_t C, dc;
  const float* g_cate; double* sumsq_out; float* sumsq_f32; float* scale; void* lws; size_t lws_bytes;
  /* plans: issued once the pinned word out.started has reached this value (steps count up; see below) */
  uint32_t plans_after;
} tlsan_static_step;
int tlsan_shard_plan_static(const tlsan_static_plan* p);
/* With TLSAN_PLAN_ASYNC in `phases` (needs s->out.started) the plans are copied and handed to ONE launch thread of the
 * library's own, which waits for the pinned word and issues them while the caller goes on with the main stream: a plan
 * is seven launches + a copy + four event operations, the step six launches, and one host thread issuing both was the
 * step's bound (85 us of HIP runtime calls per step for 77 us of kernels).  The only threading in the library (the header's
 * "single host thread per GPU" holds for every other entry point).  tlsan_shard_plans_flush() returns when the thread has
 * issued everything handed to it, with its first error if any: call it before waiting on a plan's events, before
 * touching what a queued plan writes (discarding a slot), before a stream capture, before tearing the streams down. */
int tlsan_shard_plans_flush(void);
int tlsan_shard_step_static(const tlsan_static_step* s, int32_t phases, const tlsan_static_plan* const* plans, int32_t n_plans,
                            void* stream);

/* Exclusive prefix sum + compaction of a device int32 array (the id-routing step of the sharded
 * path): prefix[k] = sum(cnt[0..k)), uniq = ascending list of k with cnt[k] > 0 and
 * prefix_nz[k]... see below.  For 0/1 flags, prefix[k] is the compact index of k.
 *   prefix  [n]  exclusive prefix of cnt
 *   uniq    [n]  (nullable) indices with cnt > 0, ascending
 *   n_uniq  [1]  (nullable) how many */
int tlsan_scan_compact(const int32_t* cnt, int32_t n, int32_t* prefix, int32_t* uniq, int32_t* n_uniq, void* stream);

/* Profiling hooks (measurement only; no reference counterpart).  level 0 = off (default),
 * 1 = HIP events around the fused forward/backward kernel of every train step,
 * 2 = events at every kernel boundary of the step.  Events are recorded on the step's stream.
 * tlsan_profile_collect waits for the recorded events and writes, per recorded step, 5 floats
 * of milliseconds {index build, fwd+bwd kernel, dK partial, dense finalize, row apply}
 * (level 1 fills only [1]); returns the number of steps written and clears the ring. */
#define TLSAN_PROF_SEGMENTS 5
int tlsan_profile_enable(int level);
/* record only every `every`-th step (default 1): timing events perturb a latency-bound pipeline */
int tlsan_profile_stride(int every);
int tlsan_profile_collect(float* host_ms, int max_steps);

/* Diagnostic: device buffer of s_memtime stamps (NULL = off, the default): entries
 * [blocks*8 waves][16] written by the fused kernel at its phase boundaries and, from entry
 * 2^20 on, [workgroups][8] written by k_apply (the buffer must hold 2^20 + 8*grid entries). */
int tlsan_debug_stamps(void* device_buf);

#ifdef __cplusplus
}
#endif
#endif /* TLSAN_H_ */
