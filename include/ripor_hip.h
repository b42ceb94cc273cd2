/*
 * ripor_hip.h — C ABI of libripor_hip.so: the MI355X (gfx950) trie-constrained beam-search
 * generative-retrieval hot path.
 *
 * The reference (HansiZeng/RIPOR) has no FFI layer: its boundary for this path is the Python call
 *   generate_for_constrained_prefix_beam_search(model, prefix_constrain_processor, input_ids,
 *       attention_mask, max_new_tokens=L, num_beams=B, num_return_sequences=B, ...)
 *   (reference t5_pretrainer/tasks/generation.py:35-78; callers t5_pretrainer/evaluate.py:60,102,149)
 * plus the constructors T5SeqAQEncoder.from_pretrained (modeling/t5_generative_retriever.py:772-855)
 * and PrefixConstrainLogitProcessorFastSparse (tasks/generation.py:603-642).
 * Each entry point below names the reference interface it replaces. The Python mirror of those
 * interfaces (ripor_amd/tasks/generation.py, ripor_amd/modeling/t5_generative_retriever.py)
 * binds these symbols with ctypes (ripor_amd/_lib.py); INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Conventions: every function returns 0 on success or a negative rpr_status; nothing throws
 * across the ABI; rpr_last_error() returns a human-readable message for the last failure on the
 * calling thread. All tensor arguments are plain pointers + sizes. Pointers marked [dev] are HIP
 * device pointers (e.g. torch tensor .data_ptr()), [host] are host pointers. Caller owns every
 * in/out buffer; the library owns its workspaces, KV cache and hipGraphs. One rpr_ctx per device,
 * not thread-safe per ctx. `stream` is a hipStream_t passed as void* (NULL = default stream).
 */
#ifndef RIPOR_HIP_H
#define RIPOR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  RPR_OK = 0,
  RPR_ERR_INVALID = -1,  /* bad argument / unsupported configuration */
  RPR_ERR_HIP = -2,      /* a HIP runtime call failed */
  RPR_ERR_NO_DEVICE = -3,
  RPR_ERR_OOM = -4
} rpr_status;

typedef struct rpr_ctx rpr_ctx;
typedef struct rpr_model rpr_model;
typedef struct rpr_trie rpr_trie;

/* Weights of a T5ForDocIDGeneration checkpoint (reference modeling/t5_generative_retriever.py:84-112;
 * SURVEY.md §8 row a14). All matrices are float32, row-major [out_features, in_features] exactly
 * as torch.nn.Linear stores them; q/k/v of one attention are concatenated along out_features by
 * the host (rows 0..inner-1 = q, then k, then v). Per-layer pointers are host arrays of device
 * pointers with num_layers / num_decoder_layers entries. */
typedef struct {
  int32_t vocab_size, d_model, d_kv, d_ff, num_heads;   /* d_kv: 64 (t5-base / t5-large) or 128 (t5-3b); every entry
                                                         * point runs both */
  int32_t num_layers, num_decoder_layers;
  int32_t rel_buckets, rel_max_distance;
  int32_t L;                     /* len(config.decoder_vocab_sizes) = max decoder positions      */
  int32_t V;                     /* decoder_vocab_sizes[i], must be equal for all i (evaluate.py:433); 2..65536 —
                                  * sizes off the 64 grid are padded internally, only rpr_debug_taps need V % 64 == 0 */
  int32_t scaleup_output_hidden; /* config.scaleup_output_hidden (t5_generative_retriever.py:427)  */
  float layer_norm_eps;
  const float* shared;           /* [dev] shared.weight [vocab_size, d_model]                     */
  const float* enc_rel_bias;     /* [dev] encoder.block.0...relative_attention_bias [buckets, H]   */
  const float* dec_rel_bias;     /* [dev] decoder.block.0...relative_attention_bias [buckets, H]   */
  const float* enc_final_ln;     /* [dev] [d_model] */
  const float* dec_final_ln;     /* [dev] [d_model] */
  const float* start_embed;      /* [dev] start_token_embed [d_model]                             */
  const float* in_embeds;        /* [dev] list_decoder_embeds stacked [L, V, d_model]              */
  const float* out_embeds;       /* [dev] list_output_embeds stacked [L, V, d_model] (== in_embeds if shared) */
  const float* dec_xkv;          /* [dev] all decoder layers' EncDecAttention k,v stacked
                                    [num_decoder_layers * 2 * inner, d_model]: layer i rows
                                    [2i*inner, (2i+1)*inner) = k, next inner rows = v               */
  const float* const* enc_ln0;   /* [host][num_layers] -> [dev] layer.0.layer_norm [d_model]       */
  const float* const* enc_qkv;   /*                    -> [dev] [3*inner, d_model]                 */
  const float* const* enc_o;     /*                    -> [dev] [d_model, inner]                   */
  const float* const* enc_ln1;
  const float* const* enc_wi;    /* [d_ff, d_model]; a gated model (rpr_load_model_ext): [2 * d_ff, d_model], wi_0 over wi_1 */
  const float* const* enc_wo;    /* [d_model, d_ff] */
  const float* const* dec_ln0;   /* [host][num_decoder_layers] */
  const float* const* dec_qkv;   /* SelfAttention [3*inner, d_model] */
  const float* const* dec_o;
  const float* const* dec_ln1;
  const float* const* dec_xq;    /* EncDecAttention.q [inner, d_model] */
  const float* const* dec_xo;    /* EncDecAttention.o [d_model, inner] */
  const float* const* dec_ln2;
  const float* const* dec_wi;
  const float* const* dec_wo;
} rpr_model_desc;

/* Arithmetic of the projection GEMMs (everything else — attention, norms, scores — is fp32/fp64):
 *  RPR_PREC_F32    exact fp32 MFMA (v_mfma_f32_32x32x2_f32), the numerical reference;
 *  RPR_PREC_F16X2  every fp32 operand carried as two f16 planes (hi + lo, 22 significant bits), products
 *                  evaluated as hi*hi + hi*lo + lo*hi with three f16 MFMAs accumulating in fp32:
 *                  fp32-equivalent to ~2^-22 at 5.3x the fp32-MFMA rate (default). */
#define RPR_PREC_F32 0
#define RPR_PREC_F16X2 1
/*  RPR_PREC_BF16   (training step only: rpr_lngknp_backward) every GEMM operand rounded to bf16, one bf16 MFMA per
 *                  product, fp32 accumulation and fp32 results — the arithmetic of the reference's bf16 autocast
 *                  (main.py:152 bf16=args.use_fp16, full_lng_knp_train_pipline.sh:93; tasks/trainer.py:229), BASELINE
 *                  config 5 as stated. The search / inference entry points need fp32-equivalent scores (1e-4) and run as
 *                  RPR_PREC_F16X2 under this setting. */
#define RPR_PREC_BF16 2

/* rpr_search flags */
#define RPR_FLAG_LOG_SOFTMAX 1u /* apply_log_softmax_for_scores (generation.py:453-455)           */
#define RPR_FLAG_NO_GRAPH 2u    /* launch kernels eagerly instead of replaying a hipGraph           */

/* Optional per-step taps for parity tests (all [dev], any may be NULL). */
typedef struct {
  float* encoder_out;   /* [Q, Lq, d_model] final encoder hidden states                            */
  float* step_logits;   /* [L, Q*B, V] logits of position t for the beams alive at step t           */
  double* step_scores;  /* [L, Q, B] cumulative float64 beam scores after step t (slot order)        */
  int32_t* step_tokens; /* [L, Q, B] token chosen for each new slot at step t                       */
  int32_t* step_parent; /* [L, Q, B] parent slot of each new slot at step t                         */
  uint64_t* step_valid; /* [L, Q, B*V/64] the trie child bitmap the selection of step t works from: bit
                           (beam*V + token) of query q is set iff token is a child of the beam's trie node —
                           the mask of PrefixConstrainLogitProcessorFastSparse.__call__ (generation.py:666-677)
                           for the beams alive at step t, in slot order                                  */
} rpr_debug_taps;

/* Timing of one kernel class, accumulated with hipEvents on the launch stream while
 * profiling is enabled (bench.py's roofline leg). */
typedef struct {
  double total_ms;
  int64_t launches;
  double flops;  /* algorithmic flops of those launches */
  double bytes;  /* algorithmic bytes of those launches */
} rpr_kernel_stats;

/* RPR_K_GEMM = the dominant projection kernel (256x256 ping-pong tiles in f16x2 mode, the fp32 MFMA kernel in exact
 * mode); RPR_K_GEMM_SMALL = the launches that fall to the 128-row / skinny tile kernels (few rows or few tiles). */
enum { RPR_K_GEMM = 0, RPR_K_DEC_SELF_ATTN = 1, RPR_K_DEC_CROSS_ATTN = 2, RPR_K_ENC_ATTN = 3,
       RPR_K_RMSNORM = 4, RPR_K_SELECT = 5, RPR_K_OTHER = 6, RPR_K_GEMM_SMALL = 7,
       RPR_K_TAIL_SELF_ATTN = 8, /* causal block attention of the forced-tail pass */
       RPR_K_FORK = 9,           /* fork classification / compaction / rank replay of the forced-tail search */
       RPR_K_COUNT = 10 };

/* ---- lifecycle (replaces: model.to(local_rank), evaluate.py:470; ddp_setup device binding) ---- */
int rpr_init(int device, rpr_ctx** out_ctx);
void rpr_free_ctx(rpr_ctx* ctx);
const char* rpr_last_error(void);
/* Library/ABI version; bumped when a signature changes or a symbol is added (4: the seq2seq step). Version 4 has since gained
 * rpr_search_margins and rpr_search_prefixes without a bump: a binding that needs one of them probes for the symbol (dlsym)
 * rather than for a version. 5: rpr_op_train_rows, the test hook of the training step's row-wise kernels. */
int rpr_abi_version(void);
/* Select the GEMM arithmetic (RPR_PREC_*); default RPR_PREC_F16X2, or RPR_PRECISION=f32|f16x2 in the
 * environment at rpr_init. Takes effect on the next rpr_search/rpr_encode/rpr_op_linear. */
int rpr_set_precision(rpr_ctx* ctx, int precision);
int rpr_get_precision(const rpr_ctx* ctx);

/* Host-only: HF T5Attention._relative_position_bucket evaluated the way the library fills its
 * device lookup tables (float32 log, truncation); rel = key_pos - query_pos. Needs no GPU. */
int rpr_rel_bucket(int rel, int bidirectional, int num_buckets, int max_distance);

/* ---- model (replaces T5SeqAQEncoder.from_pretrained(...).base_model, t5_generative_retriever.py:772-784) ---- */
int rpr_load_model(rpr_ctx* ctx, const rpr_model_desc* desc, rpr_model** out_model);
/* The same with what the desc, whose size is fixed, does not say. size = the size of this struct in bytes as the caller knows it.
 * ff_kind, the feed-forward block of every layer (HF config.feed_forward_proj):
 *   RPR_FF_RELU        "relu": wo(relu(wi x)), T5 v1.0 (DenseReluDense.wi / wo);
 *   RPR_FF_GATED_GELU  "gated-gelu": wo(gelu_new(wi_0 x) * wi_1 x), T5 v1.1 / Flan-T5 / mT5 (T5DenseGatedActDense),
 *                      gelu_new(g) = 0.5 g (1 + tanh(0.7978845608028654 (g + 0.044715 g^3))). enc_wi[i] / dec_wi[i] then point
 *                      to [2 * d_ff, d_model]: rows 0 .. d_ff-1 = wi_0 (the gate), the next d_ff rows = wi_1, concatenated by the
 *                      host like q/k/v; in rpr_param_info's order the W_in tensor of an FF sub-block is that tall tensor.
 * ext == NULL or ff_kind == RPR_FF_RELU: exactly rpr_load_model (which is this call with ext == NULL). Every entry point
 * that takes the model runs both kinds; a ReLU model enqueues what it always did. Probe for the symbol, not for a version. */
#define RPR_FF_RELU 0
#define RPR_FF_GATED_GELU 1
typedef struct { int32_t size; int32_t ff_kind; } rpr_model_ext;
int rpr_load_model_ext(rpr_ctx* ctx, const rpr_model_desc* desc, const rpr_model_ext* ext, rpr_model** out_model);
void rpr_free_model(rpr_model* model);

/* ---- trie (replaces list_smtid_to_nextids + PrefixConstrainLogitProcessorFastSparse(list, V),
 *      evaluate.py:404-434, generation.py:603-642, and smtid_to_docids, evaluate.py:439-446) ----
 * codes: [host] [N, L] row-major, codes[i*L + l] in [0, V); row i is the smtid of docid index i.
 * The library sorts the rows lexicographically (stable), keeps the sorted matrix on the device and
 * the permutation on the host. A beam's trie node is the half-open range [lo, hi) of sorted rows
 * sharing its prefix; the docids under a final smtid are perm[lo..hi). */
int rpr_build_trie(rpr_ctx* ctx, const uint16_t* codes, int64_t N, int32_t L, int32_t V, rpr_trie** out_trie);
void rpr_free_trie(rpr_trie* trie);
int64_t rpr_trie_num_rows(const rpr_trie* trie);
/* [host] perm[N]: perm[sorted_row] = original row index (docid index). Valid until rpr_free_trie. */
const int64_t* rpr_trie_perm(const rpr_trie* trie);
/* Binary trie cache replacing list_smtid_to_nextids.pkl (evaluate.py:404-408,428-432): sorted code matrix,
 * permutation and (optionally) the docid strings, so that a run needs neither the JSON parse nor the sort.
 * rpr_trie_build_file is HOST ONLY (no ctx, no GPU): the replacement of
 * `python -m t5_pretrainer.aq_preprocess.build_list_smtid_to_nextids` (aq_preprocess/build_list_smtid_to_nextids.py:13-41).
 *   keys: [host] docid strings in row order joined by '\n' (key_bytes = 0: none); src_size / src_mtime_ns: identity of
 *   the docid_to_smtid.json the codes came from (0 = unknown), returned by rpr_trie_file_info so callers can detect a
 *   stale cache. rpr_trie_load validates everything it reads (sizes vs file length, codes < V, sorted rows, perm). */
int rpr_trie_save(const rpr_trie* trie, const char* path);
int rpr_trie_build_file(const uint16_t* codes, int64_t N, int32_t L, int32_t V, const char* keys, int64_t key_bytes,
                        int64_t src_size, int64_t src_mtime_ns, const char* path);
int rpr_trie_file_info(const char* path, int64_t* N, int32_t* L, int32_t* V, int64_t* key_bytes, int64_t* src_size,
                       int64_t* src_mtime_ns);
int rpr_trie_load(rpr_ctx* ctx, const char* path, rpr_trie** out_trie);
/* HOST ONLY: the full validation rpr_trie_load performs, without a device (0 = the file is well-formed). */
int rpr_trie_file_validate(const char* path);
/* Dimensions of a trie object (the FILE's L and V after rpr_trie_load); key_bytes = size of its docid blob. */
int rpr_trie_dims(const rpr_trie* trie, int64_t* N, int32_t* L, int32_t* V, int64_t* key_bytes);
/* [host] out: key_bytes chars, the docid strings in original row order joined by '\n'. */
int rpr_trie_keys(const rpr_trie* trie, char* out);
/* A cache is built without knowing the model: widen V to the model's decoder vocab size (must exceed every code). */
int rpr_trie_set_vocab(rpr_trie* trie, int32_t V);
/* Host-side child mask of arbitrary prefixes — the processor's __call__ (generation.py:666-677)
 * without a model, for callers that use the processor object on its own. prefix: [host] [R, T] with
 * column 0 ignored (start id); out_mask: [host] [R, V] bytes 0/1. Runs a stand-alone device kernel
 * (prefix_mask_kernel: walks the prefix by binary search, then one search per token); the mask the SEARCH
 * uses is built inside select_kernel and is exposed through rpr_debug_taps.step_valid. */
int rpr_trie_mask(rpr_ctx* ctx, const rpr_trie* trie, const int32_t* prefix, int32_t R, int32_t T,
                  uint8_t* out_mask);

/* ---- docid_to_smtid.json reader (host only, no ctx) ------------------------------------------------
 * Replaces `ujson.load(docid_to_smtid_path)` + the list comprehension over 8.8 M Python lists in
 * evaluate.py:400-402,439-446 and aq_preprocess/build_list_smtid_to_nextids.py:21-27: one streaming pass
 * over {"docid": [-1, c1, ..., cL], ...} (format: aq_preprocess/create_customized_smtid_file.py:47-59)
 * into a [N, L] uint16 code matrix in file order plus the docid strings. */
typedef struct rpr_d2s rpr_d2s;
int rpr_d2s_open(const char* path, rpr_d2s** out);
/* N docs, L codes per doc (the leading -1 dropped), key_bytes = length of the '\n'-joined docid strings */
int rpr_d2s_dims(const rpr_d2s* h, int64_t* N, int32_t* L, int64_t* key_bytes);
/* codes: [host] [N, L] uint16; keys: [host] key_bytes chars ('\n'-separated, file order). Either may be NULL. */
int rpr_d2s_copy(const rpr_d2s* h, uint16_t* codes, char* keys);
void rpr_d2s_close(rpr_d2s* h);

/* ---- the hot path (replaces generate_for_constrained_prefix_beam_search, generation.py:35-251,
 *      -> beam_search_for_constrained_prefix :253-575 incl. BeamSearchScorer.process/finalize) ----
 * input_ids, attention_mask: [dev] int32 [Q, Lq] (pad id 0 / mask 0 on padding, any Lq <= 256).
 * out_tokens: [dev] int32 [Q, B, L] generated smtid tokens, beams ranked best-first per query
 *             (= outputs.sequences[:, 1:] of the reference, which prepends the start id 0).
 * out_scores: [dev] float32 [Q, B] = float32(sum of step scores (float64) / (L+1))
 *             (= outputs.sequences_scores).
 * out_row_lo/out_row_hi: [dev] int64 [Q, B] sorted-row range of each returned smtid (empty range:
 *             the smtid is not in the trie; the reference prints "smtid not in smtid_to_docid").
 * L may be smaller than the model's decoder length (prefix search, evaluate.py:134-178). */
int rpr_search(rpr_ctx* ctx, rpr_model* model, rpr_trie* trie, const int32_t* input_ids,
               const int32_t* attention_mask, int32_t Q, int32_t Lq, int32_t B, int32_t L, uint32_t flags,
               int32_t* out_tokens, float* out_scores, int64_t* out_row_lo, int64_t* out_row_hi,
               const rpr_debug_taps* taps, void* stream);

/* The same search plus its per-query PRUNING MARGIN. Every argument, every result and the work enqueued for them are those
 * of rpr_search (same bits); out_margin: [dev] float64 [Q] is written in addition (every entry, by every call).
 * Definition. At decode step t let s_t[0] >= s_t[1] >= ... be the step's candidates of one query in float64, the keys of
 * the selection: ((double)logit + (token is a trie child of the beam ? 0 : -1e9)) + beam score, the logit being the fp32
 * log-softmax value under RPR_FLAG_LOG_SOFTMAX; the padding of a logits row beyond the model's V is no candidate. The step
 * keeps ranks 0 .. B-1. gap_t = s_t[B-1] - s_t[B] if s_t[B] > -1e8 (a LIVE candidate was dropped: masked tokens and dead
 * beams carry -1e9), else +inf; an exact tie across the boundary gives 0. out_margin[q] = min over the steps of gap_t:
 * +inf = nothing live was ever dropped (the result set is the whole live candidate set), small = the choice of WHICH
 * sequences survive depended on a difference of that size at some step. The split-precision GEMMs move a cumulative score
 * by up to ~1e-4, the reference's own float32 arithmetic likewise: a query whose margin is below ~1e-3 (the test-suite's
 * PRUNE_TOL) may legitimately return a different SET of smtids than the reference; above it the set is decided.
 * Steps behind a forced-tail fork contribute nothing for the queries that left at it (all B beams live and single-sequence:
 * exactly B live candidates per later step, rank B is masked), so nothing is launched in a tail pass. The margin is
 * computed from the device's own scores: it differs from the reference's by the score error of the precision in force.
 * In the optimistic forced-tail mode the margins of a call that raised RPR_STATUS_TAIL_LEFTOVER are unspecified, like its
 * other outputs. Cost: one more kernel per selection step (one block per live query over its B * V candidates). */
int rpr_search_margins(rpr_ctx* ctx, rpr_model* model, rpr_trie* trie, const int32_t* input_ids,
                       const int32_t* attention_mask, int32_t Q, int32_t Lq, int32_t B, int32_t L, uint32_t flags,
                       int32_t* out_tokens, float* out_scores, int64_t* out_row_lo, int64_t* out_row_hi,
                       double* out_margin, const rpr_debug_taps* taps, void* stream);

/* The same search plus its beams at up to three shorter PREFIX LENGTHS (the rank-data pass runs the search at 4, 8 and
 * 16 tokens; beam search decides step by step, so the beams of a search of length p are what a longer search holds after
 * its p-th selection step). n_depths: 1..3; depths: [host] strictly ascending, each in [1, L-1]. Per prefix length p =
 * depths[k] (the four depth_* arguments are [host] arrays of n_depths [dev] pointers):
 *   depth_tokens[k]: int32 [Q, B, p], depth_scores[k]: float32 [Q, B], depth_row_lo[k] / depth_row_hi[k]: int64 [Q, B]
 * = what rpr_search(..., L = p) returns on the same trie: beams ranked by float64 sum / (p + 1), exact ties in reverse slot
 * order, float32 store, the sorted-row range of each p-prefix. The ordinary outputs are those of rpr_search(L) under the
 * same plan (same bits). Fork depths are those of the same (Q, B, L) without prefix lengths; no query is forced with
 * extras (rpr_set_tail_extras does not apply), the call is never lane-split and takes no taps. Queries walking step by
 * step at depth p are ranked by the finalize kernel on their beams; queries that left at a fork T < p by the tail pass's
 * ranking stopped at p (score at T plus the first p - T gold scores, the same additions in the same order). In the
 * optimistic forced-tail mode a call that raised RPR_STATUS_TAIL_LEFTOVER leaves these outputs unspecified too.
 * Invalid depths (unsorted, repeated, out of range, more than three) or a NULL pointer: RPR_ERR_INVALID, nothing written. */
int rpr_search_prefixes(rpr_ctx* ctx, rpr_model* model, rpr_trie* trie, const int32_t* input_ids,
                        const int32_t* attention_mask, int32_t Q, int32_t Lq, int32_t B, int32_t L, uint32_t flags,
                        int32_t* out_tokens, float* out_scores, int64_t* out_row_lo, int64_t* out_row_hi,
                        int32_t n_depths, const int32_t* depths, int32_t* const* depth_tokens, float* const* depth_scores,
                        int64_t* const* depth_row_lo, int64_t* const* depth_row_hi, void* stream);

/* Lane split of large batches. A call of rpr_search with at least `min_rows` decoder rows (queries x beams; default
 * 10240; 0 = never; env RPR_LANE_MIN_ROWS) runs as two halves on two internal HIP streams, each confined to half of the CUs
 * (hipExtStreamCreateWithCUMask) and each with its own workspace: the HBM-bound attention of one half overlaps the
 * power-bound GEMMs of the other (+3.6 % queries/s at 2150 queries in flight; on one stream all CUs are in the same
 * phase). Results are identical to the unsplit call; the caller's stream waits for both halves. Calls with debug taps
 * are never split. rpr_lane_split returns the threshold in force, 0 when splitting is off or masked streams are
 * unavailable on the device. No counterpart in the reference (its loop is host-bound at batch 1). */
int rpr_set_lane_split(rpr_ctx* ctx, int32_t min_rows);
int32_t rpr_lane_split(rpr_ctx* ctx);

/* Forced-tail evaluation (default on; env RPR_FORCED_TAIL=0 / RPR_FORK_DEPTHS="4,6"). Beam search over a docid trie
 * stops deciding early: once every beam of a query stands on a trie node under which a single distinct smtid remains
 * (8.8 M docs under 256^4 depth-4 prefixes: after 4 steps for 99 % of the queries), each beam has exactly one valid
 * child per step, nothing can be pruned any more and the remaining tokens are the rest of the beam's code row — only
 * the scores are missing. rpr_search therefore walks the first steps sequentially, FORKS at up to two depths chosen from
 * the trie (queries that are forced there leave; the others are compacted and walk on), and scores the remaining
 * positions of the forced queries in one teacher-forced decoder pass per fork instead of L - T KV-gathering steps.
 * Results are those of the step-by-step loop (generation.py:423-540: float64 cumulative scores, the slot order of every
 * step replayed, sum/(L+1) finalize with ties in reverse slot order); a fork only takes a query whose beams are all
 * live, single-sequence and close enough in score that no masked (-1e9) candidate could be selected (bound on |logit|
 * from the output codebooks, computed at rpr_load_model). Calls with debug taps never fork; RPR_FLAG_LOG_SOFTMAX
 * forks too (the tail pass then computes the V logits of every forced position for the log-sum-exp).
 *   rpr_set_forced_tail(ctx, mode)           0 = off; 1 = exact (default): whoever is still unforced after the last fork
 *                                            walks on to L on the device; 2 = optimistic: when the trie statistics promise
 *                                            an (almost always) empty last stage, it is not enqueued at all (~100 launches
 *                                            per remaining step for nobody) — a query left unforced by the last fork raises
 *                                            the sticky RPR_STATUS_TAIL_LEFTOVER and the results of that call are NOT valid:
 *                                            repeat it in mode 1 (ripor_amd/tasks/generation.py and bench.py do).
 *   rpr_forced_tail(ctx)                     the mode in force;
 *   rpr_set_fork_depths(ctx, n, depths)      n = -1: depths from the trie statistics (default); n = 0..2: explicit,
 *                                            ascending, each in [1, L-1] (entries >= L are ignored at search time);
 *   rpr_fork_depths(...)                     the depths a search of this shape would use -> out_depths[2]; returns
 *                                            their number (>= 0) or a negative rpr_status. */
int rpr_set_forced_tail(rpr_ctx* ctx, int32_t mode);
int32_t rpr_forced_tail(const rpr_ctx* ctx);
int rpr_set_fork_depths(rpr_ctx* ctx, int32_t n, const int32_t* depths);
int rpr_fork_depths(rpr_ctx* ctx, rpr_model* model, rpr_trie* trie, int32_t Q, int32_t B, int32_t L, uint32_t flags,
                    int32_t* out_depths);
/* Layer-0 Q/K/V table. The decoder's input row at layer 0 depends on (position, token) alone, so its self-attention
 * projection does too: in RPR_PREC_F16X2 the first rpr_search of a model makes the L * V + 1 rows of q | k | v once (on
 * the device, by the projection kernel itself), and the searches read rows of it where they would launch that projection
 * through the 256 x 256 tile kernel; results are the same bits. rpr_adamw_step and rpr_set_precision drop the table (the
 * next search makes it again); a model whose table would exceed 160 MiB (t5-3b at 32 x 256) keeps the projection.
 *   rpr_set_l0_table(ctx, mode)      0 = never, 1 = as above (default), 2 = for every such launch of a search, whatever
 *                                    kernel it would have taken (tests: scores then differ by that kernel's rounding);
 *   rpr_l0_table_bytes(ctx, model)   size of the model's table if the next search on this ctx may read it, else 0. */
int rpr_set_l0_table(rpr_ctx* ctx, int32_t mode);
int64_t rpr_l0_table_bytes(const rpr_ctx* ctx, const rpr_model* model);
/* MFMA shape of the 256 x 256 split-precision GEMM kernel (RPR_PREC_F16X2): 0 = v_mfma_f32_32x32x16_f16 everywhere,
 * 1 (default) = v_mfma_f32_16x16x32_f16 in the forced-tail passes of rpr_search / rpr_search_margins, which hold most of
 * a large search's GEMM time. Same tiles, same three products per element; a K-tile's 32 columns are summed in another
 * order, so the scores of forced sequences move in their last bits (<= 3e-5). The encoder, the sequential steps, the
 * layer-0 table and the projection it replaces keep the 32x32x16 arithmetic and its bits, and with them every pruning
 * decision of the steps; so do the training step, rpr_encode, the cross-encoder and the bf16 GEMMs. One pruning decision
 * does see the tail pass's rounding on either shape: a query forced with extras (rpr_set_tail_extras) keeps the best
 * num_beams of its num_beams + extras sequences by their tail scores, so a tie closer than that rounding may fall
 * differently at 0 and at 1. */
int rpr_set_gemm_mfma16(rpr_ctx* ctx, int32_t mode);
int32_t rpr_gemm_mfma16(const rpr_ctx* ctx);
/* HOST ONLY (no ctx, no GPU): the statistic the automatic fork depths come from. codes: [host] [N, Lc] in any order;
 * out_frac: [host] L + 1 doubles, out_frac[t] = share of the trie nodes at depth t (distinct t-prefixes) under which
 * exactly one distinct L-token sequence remains. A query whose B beams stand on random depth-t nodes is forced with
 * probability ~ out_frac[t]^B: the first fork is the first depth where that reaches 1/2, the second the first later
 * depth where fewer than 0.05 queries of the call are expected to stay unforced. */
int rpr_trie_single_frac(const uint16_t* codes, int64_t N, int32_t Lc, int32_t L, double* out_frac);
/* HOST ONLY: from the same pass, out_mean[t] (L + 1 doubles) = the mean over the depth-t nodes of (distinct L-token
 * sequences under the node - 1): what a fork that takes queries with a few extra sequences along (rpr_set_tail_extras)
 * has to carry per beam. Duplicated smtids count once. */
int rpr_trie_extra_mean(const uint16_t* codes, int64_t N, int32_t Lc, int32_t L, double* out_mean);
/* HOST ONLY: the fork depths the library derives from those two statistics (L + 1 doubles each) for a search of Q
 * queries, B beams, L tokens under rpr_set_forced_tail mode `forced_tail` and rpr_set_tail_extras mode `tail_extras`;
 * out_depths: 2 entries; *out_drop_last = 1 when no stage follows the last fork (optimistic mode). Returns the number of
 * forks. Explicit depths (rpr_set_fork_depths) and the model's logit bound are not part of it. */
int rpr_plan_forks(const double* single_frac, const double* extra_mean, int32_t Q, int32_t B, int32_t L, int32_t forced_tail,
                   int32_t tail_extras, int32_t* out_depths, int32_t* out_drop_last);
/* Forced with extras: at a fork, a query whose beams hold a few distinct sequences more than one each (at most n over all
 * its beams) is forced as well — the extra sequences ride through the same tail pass in a spare entry and the remaining
 * selection steps of the query are replayed on its B + extras candidates, pruning included. Results are those of the
 * step-by-step loop. mode: -1 = automatic (default: searches with more than 4096 decoder rows and fewer than 32 beams,
 * n = 4), 0 = off, 1..31 = always, with budget n (never with 32 beams or more, nor in rpr_search_margins). Part of the
 * key of the captured graphs. */
int rpr_set_tail_extras(rpr_ctx* ctx, int32_t mode);
int32_t rpr_tail_extras(const rpr_ctx* ctx);
/* Diagnostic (synchronises the device): for every fork of the last rpr_search its depth, the number of queries that
 * were forced there and the number that walked on; [host] arrays of 2 entries each; returns the number of forks. */
int rpr_last_fork_stats(rpr_ctx* ctx, int32_t* out_depths, int32_t* out_forced, int32_t* out_left);

/* ---- forward of the prefix-oriented ranking fine-tune step (BASELINE config 5) ----------
 * Replaces the forward of T5SeqAQEncoderForLngKnpMarginMSE (modeling/t5_generative_retriever.py:902-966; also
 * T5SeqAQEncoderForMarginMSE :847-882 with n_prefix = 1 and T5SeqAQEncoder.rerank_forward :788-792 with n_prefix = 0):
 * teacher-forced decoder passes of base_model over the smtids of n_docs documents per query
 * (decoder_input_ids = [-1, c_1 .. c_{L-1}], dataset/dataset.py:497-500), decode() of the doc encodings through the
 * OUTPUT codebooks (:812-826), per-position scores <decoder_last_hidden_state[i], E_out[i][c_i]>, and the MSE losses
 * between the student margins over the first prefix_lens[p] positions and the teacher margins.
 *   input_ids, attention_mask: [dev] int32 [bz, Lq]      (the query; the positive and the negative pass share it)
 *   doc_codes:   [dev] int32 [bz, n_docs, L]   doc_codes[b][0] = positive, [b][1] = negative smtid (codes in [0, V))
 *   teacher_pos, teacher_neg: [dev] float [n_prefix, bz]  teacher scores per prefix length (row p belongs to
 *                prefix_lens[p]; the reference's order is rank (= L), rank_4, rank_8, rank_16)
 *   prefix_lens: [dev] int32 [n_prefix]
 *   out_losses:  [dev] float [n_prefix]        mean_b (student_margin - teacher_margin)^2   (torch.nn.MSELoss)
 *   out_position_scores: [dev] float [bz, n_docs, L], nullable
 * Inference-style forward (split-precision GEMMs, nothing kept for a backward pass); the training step is
 * rpr_lngknp_backward + rpr_adamw_step below. Eager launches on `stream`; asynchronous. Lq <= 256; d_kv 64 or 128 (128-dim
 * heads run on the attention kernels of the search path: enc_attn_kernel<128>, dec_cross_attn_block_kernel<128>). */
int rpr_lngknp_forward(rpr_ctx* ctx, rpr_model* model, const int32_t* input_ids, const int32_t* attention_mask,
                       int32_t bz, int32_t Lq, const int32_t* doc_codes, int32_t n_docs, int32_t L,
                       const float* teacher_pos, const float* teacher_neg, const int32_t* prefix_lens, int32_t n_prefix,
                       float* out_losses, float* out_position_scores, void* stream);

/* ---- the training step of the same model (config 5): backward pass + optimizer --------------------------------
 * Replaces, for loss_type t5seq_aq_encoder_lng_knp_margin_mse, what HF Trainer does per step around the forward above
 * (tasks/trainer.py:203-275 training_step: loss = sum of the task losses, loss.backward(); Trainer defaults behind
 * main.py:131-155: clip_grad_norm_(1.0), torch.optim.AdamW(lr, betas (0.9, 0.999), eps 1e-8, weight_decay 0)).
 *
 * Trainable tensors and the flat buffers. The model's tensors (the device pointers of rpr_model_desc: fp32, caller
 * owned) are updated IN PLACE by rpr_adamw_step. Gradients and the two AdamW moments live in caller-owned flat fp32
 * buffers of rpr_param_total(model) elements; tensor i occupies [offset_i, offset_i + numel_i) in each of them and
 * rpr_param_info returns its device pointer (so the host can map it back to a checkpoint name), numel and offset.
 * Order: shared, encoder / decoder relative bias, final layer norms, start embedding, stacked input codebooks, stacked
 * output codebooks (absent when shared with the input ones), stacked cross-attention k/v, then per encoder layer
 * ln0, qkv, o, ln1, wi, wo and per decoder layer ln0, qkv, o, ln1, xq, xo, ln2, wi, wo (the concatenated layouts of
 * rpr_model_desc). The flat gradient buffer is what a data-parallel caller all-reduces (RCCL) between the two calls.
 *
 * rpr_lngknp_backward: forward (activations kept in library-owned memory) + backward of the sum of the n_prefix
 *   margin-MSE losses; same batch arguments as rpr_lngknp_forward with n_docs = 2; writes out_losses [dev, n_prefix]
 *   and overwrites flat_grads [dev, rpr_param_total]. fp32 activations and gradients; the matrix products follow the
 *   context's precision (rpr_set_precision): RPR_PREC_F16X2 (default) = split-precision f16 MFMA with per-tensor
 *   dynamic plane scales found on the device, RPR_PREC_F32 = exact-fp32 MFMA. Deterministic reductions in both.
 *   Lq <= 256, L <= the model's decoder length; d_kv 64 or 128. Up to self-attention max(L, Lq) <= 91 and cross-attention
 *   130 (2 L + Lq) + 4 L (Lq + 1) + Lq <= 40960 floats (L 32 with Lq <= 91) the attention backward holds one (sequence,
 *   head) in the 160 KB of LDS of a CU, 128-dim heads 64 columns at a time in the same carve. Beyond, 64-dim heads go on in
 *   32-row tiles up to Lq = 256 (these passes too, and the dropped-out forward); 128-dim heads are RPR_ERR_INVALID there,
 *   as is Lq > 256, before anything is enqueued.
 * rpr_adamw_step: global L2 norm of flat_grads (-> out_grad_norm [dev, 1], nullable), clip coefficient
 *   min(1, max_grad_norm / (norm + 1e-6)) (max_grad_norm <= 0: no clipping), AdamW update of every tensor with the
 *   bias corrections of `step` (1-based); the f16 weight planes of the search / inference paths are marked stale and
 *   re-split by the next rpr_search / rpr_lngknp_forward / rpr_encode on this model (a training loop never pays for it). weight_decay applies to every tensor except the two relative-attention-bias tables (HF 4.17
 *   Trainer.create_optimizer excludes nn.LayerNorm parameters and names containing "bias"; T5LayerNorm is not an
 *   nn.LayerNorm there, so layer-norm weights decay). The reference's default is weight_decay = 0.
 *   exp_avg / exp_avg_sq: [dev, rpr_param_total], zero before the first step. */
int64_t rpr_param_count(rpr_model* model);
int64_t rpr_param_total(rpr_model* model);
int rpr_param_info(rpr_model* model, int64_t index, const float** ptr, int64_t* numel, int64_t* offset);
int rpr_lngknp_backward(rpr_ctx* ctx, rpr_model* model, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz,
                        int32_t Lq, const int32_t* doc_codes, int32_t L, const float* teacher_pos, const float* teacher_neg,
                        const int32_t* prefix_lens, int32_t n_prefix, float* out_losses, float* flat_grads, void* stream);
/* The same pass with the gradient exchange overlapped (reference: DistributedDataParallel's bucketed all-reduce running
 * under the backward pass, tasks/trainer.py:486). The flat gradient buffer is handed over in BUCKETS: one per
 * transformer layer (decoder layers last to first, then encoder layers last to first: the order the backward finishes
 * them; a layer's tensors are contiguous in the flat layout) and a final one for everything in front of the first layer
 * (embeddings, codebooks, cross K/V, final norms, bias tables). For each bucket the library makes `comm_stream` wait for
 * the kernels that produce it (main stream and the internal weight-gradient stream) and then calls, on the calling host
 * thread and before returning, on_bucket(user, offset, numel): the callback enqueues the bucket's all-reduce (RCCL) on
 * comm_stream, where it runs beside the remaining backward kernels. The caller joins comm_stream before rpr_adamw_step.
 * on_bucket == NULL: exactly rpr_lngknp_backward. */
typedef void (*rpr_grad_bucket_cb)(void* user, int64_t offset, int64_t numel);
int rpr_lngknp_backward_buckets(rpr_ctx* ctx, rpr_model* model, const int32_t* input_ids, const int32_t* attention_mask,
                                int32_t bz, int32_t Lq, const int32_t* doc_codes, int32_t L, const float* teacher_pos,
                                const float* teacher_neg, const int32_t* prefix_lens, int32_t n_prefix, float* out_losses,
                                float* flat_grads, void* stream, void* comm_stream, rpr_grad_bucket_cb on_bucket, void* user);
/* ---- the seq2seq docid cross-entropy step (loss_type t5seq_aq_encoder_seq2seq; the first stage of RIPOR's docid training) --
 * Replaces T5SeqAQEncoderForSeq2Seq (modeling/t5_generative_retriever.py:968-1019): the teacher-forced decoder over ONE
 * sequence per query, decoder_input_ids = [-1, labels[:, :-1]] (dataset/dataset.py:527-550), logits[:, i] = h[:, i] E_i^T with
 * h = decoder_last_hidden_state (final RMSNorm, scaleup_output_hidden included) and E_i the output codebook of position i (the
 * input codebook when shared), loss = nn.CrossEntropyLoss over the bz * L rows (their mean). The encoder / decoder GEMMs follow
 * rpr_set_precision like rpr_lngknp_backward; the head (logits, log-softmax, cross-entropy, its gradients) is exact fp32 in
 * every mode. Deterministic: two identical calls give bit-identical losses and gradients.
 *   input_ids, attention_mask: [dev] int32 [bz, Lq]   (Lq <= 256)
 *   labels:      [dev] int32 [bz, L]   codes in [0, V): a label outside is RPR_ERR_INVALID (checked on the host before anything
 *                is enqueued: one copy of bz * L labels and a synchronisation of `stream`)
 *   out_loss:    [dev] float [1]
 *   out_label_logprob: [dev] float [bz, L], nullable: log-softmax of each position's logits at its label
 * Limits: d_kv 64 or 128 and the LDS admission of rpr_lngknp_backward (one document per query), L <= the model's L,
 * V % 64 == 0 and V <= 1024, d_model % 32 == 0.
 * rpr_seq2seq_forward: the forward and the head only. rpr_seq2seq_backward: forward + backward, overwrites flat_grads
 * [dev, rpr_param_total] (same layout and optimizer step as the ranking step: rpr_adamw_step).
 * rpr_seq2seq_backward_buckets: the same with the gradient buckets of rpr_lngknp_backward_buckets (same order, same layout). */
int rpr_seq2seq_forward(rpr_ctx* ctx, rpr_model* model, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz,
                        int32_t Lq, const int32_t* labels, int32_t L, float* out_loss, float* out_label_logprob, void* stream);
int rpr_seq2seq_backward(rpr_ctx* ctx, rpr_model* model, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz,
                         int32_t Lq, const int32_t* labels, int32_t L, float* out_loss, float* flat_grads, void* stream);
int rpr_seq2seq_backward_buckets(rpr_ctx* ctx, rpr_model* model, const int32_t* input_ids, const int32_t* attention_mask,
                                 int32_t bz, int32_t Lq, const int32_t* labels, int32_t L, float* out_loss, float* flat_grads,
                                 void* stream, void* comm_stream, rpr_grad_bucket_cb on_bucket, void* user);
/* ---- the dense first-stage step (loss_type t5seq_pretrain_margin_mse; the first model of the RIPOR pipeline) ----------------
 * Replaces T5SeqPretrainEncoder.forward (modeling/t5_generative_retriever.py:708-757) in the case its training scripts run:
 * decoder_input_ids = [-1], no commit loss. rep(x) = decoder_last_hidden_state[:, 0] of the encoder plus one decoder position
 * fed with the start embedding (final RMSNorm and scaleup_output_hidden included: what rpr_embed computes),
 *   margin_b = <rep(q_b), rep(d+_b)> - <rep(q_b), rep(d-_b)>,  loss = mean_b (margin_b - (teacher_pos_b - teacher_neg_b))^2.
 * The query is encoded once and receives both gradient contributions (the reference passes the same text twice).
 *   input_ids, attention_mask: [dev] int32 [3, bz, Lt]: group 0 the queries, 1 the positive, 2 the negative documents, all
 *                      padded to one Lt <= 256; a sequence with an all-zero mask sets the empty-query status bit
 *   teacher_pos, teacher_neg: [dev] float [bz]
 *   out_loss:          [dev] float [1]
 *   out_scores:        [dev] float [bz, 2], nullable: the two dot products of every example
 *   out_reps:          [dev] float [3 bz, d_model], nullable: the representations, in the order of input_ids
 * Limits: bz >= 1, d_kv 64 (Lt <= 256) or 128 (Lt <= 91), else RPR_ERR_INVALID before anything is enqueued. The head is exact
 * fp32 in every precision mode and deterministic.
 * rpr_dense_mse_forward: evaluation mode. rpr_dense_mse_backward: forward + backward, overwrites flat_grads [dev,
 * rpr_param_total] (layout and optimizer step of the other training steps; the codebooks get exactly zero);
 * rpr_set_train_dropout applies. rpr_dense_mse_backward_buckets: the same with the gradient buckets of
 * rpr_lngknp_backward_buckets. (Added to ABI version 4 without a bump, as rpr_search_margins was: probe for the symbol.) */
int rpr_dense_mse_forward(rpr_ctx* ctx, rpr_model* model, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz,
                          int32_t Lt, const float* teacher_pos, const float* teacher_neg, float* out_loss, float* out_scores,
                          float* out_reps, void* stream);
int rpr_dense_mse_backward(rpr_ctx* ctx, rpr_model* model, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz,
                           int32_t Lt, const float* teacher_pos, const float* teacher_neg, float* out_loss, float* flat_grads,
                           void* stream);
int rpr_dense_mse_backward_buckets(rpr_ctx* ctx, rpr_model* model, const int32_t* input_ids, const int32_t* attention_mask,
                                   int32_t bz, int32_t Lt, const float* teacher_pos, const float* teacher_neg, float* out_loss,
                                   float* flat_grads, void* stream, void* comm_stream, rpr_grad_bucket_cb on_bucket, void* user);
int rpr_adamw_step(rpr_ctx* ctx, rpr_model* model, const float* flat_grads, float* exp_avg, float* exp_avg_sq, int64_t step,
                   float lr, float beta1, float beta2, float eps, float weight_decay, float max_grad_norm,
                   float* out_grad_norm, void* stream);
/* Dropout of the two training steps (the reference trains in model.train(): every dropout of HF T5Stack is live at the
 * checkpoint's dropout_rate — stack input, attention probabilities, sub-block outputs, the feed-forward's inner activation,
 * stack output; both stacks). Applies to the rpr_lngknp_backward[_buckets], rpr_seq2seq_backward[_buckets] and
 * rpr_dense_mse_backward[_buckets] calls that follow, until set again; rpr_lngknp_forward, rpr_seq2seq_forward,
 * rpr_dense_mse_forward, rpr_search*, rpr_encode and rpr_embed stay in evaluation mode.
 * 0 <= rate < 1, else RPR_ERR_INVALID; the default, rate 0, is off: a training call then enqueues exactly what it enqueues
 * without this call. The mask of an element is a stateless function of (seed, step, site, logical coordinates) — Philox4x32-10,
 * csrc/dropout.h, DESIGN.md "Dropout in the training step" — so the same (seed, step) gives the same bits in every precision
 * mode and launch shape, and nothing but (seed, step) has to be kept to resume a run. The encoder runs once per query: the
 * positive and the negative pass share its masks (the reference runs it twice, with independent masks). */
int rpr_set_train_dropout(rpr_ctx* ctx, float rate, uint64_t seed, uint64_t step);

/* ---- sticky status of a ctx ------------------------------------------------------------------------
 * RPR_STATUS_SATURATED: in RPR_PREC_F16X2 mode an activation left the range of the f16 planes (|x| > 65504 after
 *   the plane scale: 4094 for normalised activations and attention outputs, 65504 for the residual stream, 1.05e6
 *   for the FF intermediate) and was clamped — the results of the searches since the last clear are NOT trustworthy;
 *   repeat them with rpr_set_precision(RPR_PREC_F32) (ripor_amd/tasks/generation.py does so automatically).
 *   Weights are checked at rpr_load_model: a model that does not fit is pinned to RPR_PREC_F32 (rpr_model_f32_only).
 * RPR_STATUS_EMPTY_QUERY: a query's attention mask has no attended position (its cross-attention output is defined
 *   as zero here; the reference would average the padded positions).
 * RPR_STATUS_SMALL_STREAM: in RPR_PREC_F16X2 mode a row of the residual stream had an RMS under 2^-3 (0 < mean(x^2) < 2^-6)
 *   at one of the pass's RMSNorm sites (tested once per pass over its row totals). The planes of the stream and its fixed-point row sums have ABSOLUTE resolutions (2^-21 per
 *   element, 2^-17 per 16- to 256-column piece of a row) that were chosen for rows of RMS ~1 .. 1e5; under the floor the
 *   normalised activations lose their fifth digit and beam scores leave the 1e-4 bar (measured: DESIGN.md, "Working range").
 *   Nothing is clamped, but the results since the last clear are NOT trustworthy: repeat them with
 *   rpr_set_precision(RPR_PREC_F32), as after RPR_STATUS_SATURATED (the Python boundaries do). Rows of zeros do not raise it.
 * rpr_get_status synchronises `stream`, returns the flags accumulated by the work enqueued so far and, if clear != 0,
 * resets them. */
#define RPR_STATUS_SATURATED 1u
#define RPR_STATUS_EMPTY_QUERY 2u
/* RPR_STATUS_TAIL_LEFTOVER: a search in the optimistic forced-tail mode (rpr_set_forced_tail(ctx, 2)) met a query that
 *   was still unforced at its last fork; the outputs of that query are unspecified — repeat the call in mode 1. */
#define RPR_STATUS_TAIL_LEFTOVER 4u
#define RPR_STATUS_SMALL_STREAM 8u
int rpr_get_status(rpr_ctx* ctx, void* stream, uint32_t* out_flags, int clear);
/* The same words WITHOUT a synchronisation: enqueues on `stream` a copy of the four raw status words ([0] != 0:
 * SATURATED, [1] != 0: EMPTY_QUERY, [2] != 0: TAIL_LEFTOVER, [3] != 0: SMALL_STREAM) into host_words ([host], pinned, 16 bytes;
 * NULL = no copy) and, if clear != 0, their reset behind it. A caller that records an event after this call reads the
 * flags of exactly the work enqueued before it once the event has completed — the search loop of
 * ripor_amd/evaluate.py checks batch n this way while batch n + 1 runs (the reference loop synchronises >= 2*B*Q times
 * per step). */
int rpr_status_words_async(rpr_ctx* ctx, void* stream, uint32_t* host_words, int clear);
int rpr_model_f32_only(const rpr_model* model);

/* ---- measurement ---- */
/* Enable/disable per-kernel-class hipEvent timing (forces eager launches while enabled). */
int rpr_profile_enable(rpr_ctx* ctx, int enable);
int rpr_profile_reset(rpr_ctx* ctx);
/* Synchronises the recorded events and returns the accumulated statistics for one class. */
int rpr_profile_get(rpr_ctx* ctx, int kernel_class, rpr_kernel_stats* out);
/* Bytes of device memory the ctx currently holds for workspaces + KV cache. */
int64_t rpr_workspace_bytes(const rpr_ctx* ctx);

/* ---- single-operator entry points (kernel-level parity tests; same kernels the search uses) ---- */
/* C[M,N] = act(A[M,K] @ W[N,K]^T) (+ residual[M,N]); fp32 MFMA. K % 32 == 0, N % 32 == 0. */
int rpr_op_linear(rpr_ctx* ctx, const float* A, const float* W, const float* residual, float* C,
                  int32_t M, int32_t N, int32_t K, int32_t relu, void* stream);
/* The bf16 GEMM kernels of the fine-tune step (RPR_PREC_BF16; row f4), as a kernel-level parity hook: operands rounded to
 * bf16, one bf16 MFMA per product, fp32 accumulation. n_products = 0: C[M,N] = act(A W^T) (+ residual) through the step's
 * own kernel choice (128-row LDS-DMA tiles, 256x256 ping-pong tiles, split-K for long reductions into few tiles).
 * n_products = 1..8: the grouped launch of the weight-gradient products (gemm_h2_pp_group_kernel, one K-loop per tile):
 * product i = rows [0, M - 256 i) of A against W, written to C + i * M * N (row stride N); residual and relu must be 0.
 * K % 64 == 0. Reference arithmetic: torch bf16 autocast matmul with fp32 accumulation (tasks/trainer.py:229). */
/* Test hook: one RPR_PREC_F16X2 launch C = A[M,K] W[N,K]^T with one of the epilogues a search gives its projections, on the
 * MFMA shape asked for (mfma16: 0 = 32x32x16, 1 = 16x16x32 where the launch takes the 256 x 256 kernel). All pointers [dev].
 *   RPR_LIN_F32         out0 [M,N] = relu?(C) + resid (resid nullable)
 *   RPR_LIN_X_PLANES    residual stream: resid [M,N] is split into out_planes ([2][M][N] f16, scale 1/16) first, then
 *                       out_planes = planes(resid + C) in place and ssq_out[m] += 65536 * sum_n x[m,n]^2 (fixed point; the caller
 *                       zeroes it)
 *   RPR_LIN_FF_PLANES   out_planes = planes(relu(C)), scale 1/16
 *   RPR_LIN_KV_SCATTER  columns [0, split_n) -> out0 [M, split_n]; the next two blocks of split_n columns -> out1 / out2 in
 *                       the K/V-cache layout: element (m, n) at (m / rm_B) * (split_n / 64) * rm_B * 64 + (n / 64) * rm_B * 64 +
 *                       (m % rm_B) * 64 + n % 64
 *   RPR_LIN_FUSED_NORM  A = the un-normalised stream: out0[m, :] = C[m, :] * rsqrt(row_ssq[m] / (65536 K) + eps)
 *   RPR_LIN_LIVE_ROWS   out0 rows [0, *m_dev) = C; rows from *m_dev on are not written */
#define RPR_LIN_F32 0
#define RPR_LIN_X_PLANES 1
#define RPR_LIN_FF_PLANES 2
#define RPR_LIN_KV_SCATTER 3
#define RPR_LIN_FUSED_NORM 4
#define RPR_LIN_LIVE_ROWS 5
int rpr_op_linear_h2(rpr_ctx* ctx, const float* A, const float* W, int32_t M, int32_t N, int32_t K, int32_t mode, int32_t mfma16,
                     int32_t relu, const float* resid, const uint64_t* row_ssq, float eps, const int32_t* m_dev, int32_t rm_B,
                     int32_t split_n, float* out0, float* out1, float* out2, void* out_planes, uint64_t* ssq_out, void* stream);
int rpr_op_linear_bf16(rpr_ctx* ctx, const float* A, const float* W, const float* residual, float* C,
                       int32_t M, int32_t N, int32_t K, int32_t relu, int32_t n_products, void* stream);
/* out[rows,d] = w * x * rsqrt(mean(x^2) + eps) */
int rpr_op_rmsnorm(rpr_ctx* ctx, const float* x, const float* w, float* out, int32_t rows, int32_t d,
                   float eps, void* stream);
/* The activation dropout mask of the training step over x [n_seq, n_pos, n_feat] (out may be x): out = 0 where the element's
 * draw is below round(rate * 2^32), x * fp32(1 / (1 - rate)) elsewhere. n_pos <= 65536, 0 <= site < 65536. The parity hook of
 * the device mask against its numpy restatement (tests/dropout_mask.py). */
int rpr_op_dropout(rpr_ctx* ctx, const float* x, float* out, int64_t n_seq, int32_t n_pos, int32_t n_feat, float rate,
                   uint64_t seed, uint64_t step, int32_t site, void* stream);
/* The gate of a gated-GELU feed-forward block (RPR_FF_GATED_GELU), the kernel the passes launch behind the W_in product.
 * gu: [dev] fp32 [M, 2F], columns 0..F-1 = g (the wi_0 half), F..2F-1 = u (the wi_1 half); y = gelu_new(g) * u, [M, F].
 *   out_f32 (nullable): y as fp32 [M, F] (what the exact-fp32 mode writes);
 *   out_planes (nullable): the two f16 planes [2][M][F] of y / 16 (the split mode's FF operand; a |y| beyond 1.05e6 is clamped
 *                 and raises RPR_STATUS_SATURATED like the ReLU epilogue's planes);
 *   m_dev (nullable): [dev] int32 live row count: rows from *m_dev on are neither read nor written.
 * F % 4 == 0, M >= 1. */
int rpr_op_gated_gelu(rpr_ctx* ctx, const float* gu, int32_t M, int32_t F, const int32_t* m_dev, float* out_f32, void* out_planes,
                      void* stream);
/* Its backward (training walk): dgu [M, 2F] = (dmid * u * gelu_new'(g) | dmid * gelu_new(g)) from gu [M, 2F] and dmid [M, F],
 * gelu_new'(g) = 0.5 (1 + t) + 0.5 g (1 - t^2) c (1 + 3 * 0.044715 g^2), t = tanh(c (g + 0.044715 g^3)), c = 0.7978845608028654.
 * fp32 in every precision mode, one thread per element group, no atomics: two calls give the same bits. */
int rpr_op_gated_gelu_bwd(rpr_ctx* ctx, const float* gu, const float* dmid, int32_t M, int32_t F, float* dgu, void* stream);
/* ---- attention test hooks: one launch of an attention site of the search path, routed by the site's own launcher ----
 * Every hook fills the site's argument struct from the descriptor, asks the site's planner and runs the site's launcher, so
 * the shape takes the kernel a search would give it; *out_kernel (nullable) receives the AttnKernel the plan chose (its name:
 * rpr_attn_kernel_name). A shape the planner refuses returns RPR_ERR_INVALID with a message and launches nothing. All
 * pointers are [dev]; the relative-position bucket tables are built from num_buckets / max_distance as at model load.
 * Output: fp32 `out`, or — when out_planes is set — the two f16 planes of out * 16 at out_planes and out_planes +
 * plane_stride (elements), rows laid out as the fp32 output; a clamped plane value raises RPR_STATUS_SATURATED on the ctx.
 * Scores are unscaled: softmax(q . k + bias[bucket(rel)]) . v over the attended keys. dkv = 64 or 128. */
typedef struct rpr_enc_attn_op {
  const float* qkv;         /* [rows, 3 * H * dkv]: q | k | v; padded: rows = Q * Lq; packed: row offs[q] + i */
  const int32_t* mask;      /* [Q, Lq] key mask (NULL with causal) */
  const float* rel_bias;    /* [num_buckets, H] */
  const int32_t* offs;      /* nullable (packed rows): first row of query q ... */
  const int32_t* lens;      /*   ... and its row count (index of the last attended key + 1) */
  float* out;               /* [rows, H * dkv] */
  void* out_planes;
  int64_t plane_stride;
  int32_t num_buckets, max_distance, Q, Lq, H, dkv;
  int32_t causal;           /* 1: key j <= query i only, unidirectional buckets (teacher-forced decoder), Lq <= 64 */
  int32_t mfma;             /* EncAttnArgs::mfma of the training forward */
} rpr_enc_attn_op;
int rpr_op_enc_attn(rpr_ctx* ctx, const rpr_enc_attn_op* op, int32_t* out_kernel, void* stream);
/* Self-attention of sequential step t: row r = q * B + b attends to positions 0..t of its ancestry; the dkv floats of
 * (query, head, position p, slot) start at q * q_stride + head * h_stride + p * pos_stride + slot * slot_stride, slot =
 * anc[r * anc_ld + p] for p < t and b for p = t. Queries from *nq_dev on (nullable) are skipped. */
typedef struct rpr_dec_self_attn_op {
  const float* q;           /* [Q * B, H * dkv] */
  const float* kcache;
  const float* vcache;
  const uint16_t* anc;
  const float* rel_bias;    /* [num_buckets, H] */
  const int32_t* nq_dev;
  float* out;               /* [Q * B, H * dkv] */
  void* out_planes;
  int64_t plane_stride, q_stride, h_stride, pos_stride, slot_stride;
  int32_t anc_ld, num_buckets, max_distance, Q, B, H, t, dkv;
} rpr_dec_self_attn_op;
int rpr_op_dec_self_attn(rpr_ctx* ctx, const rpr_dec_self_attn_op* op, int32_t* out_kernel, void* stream);
/* Cross-attention of B rows per query against the query's Lq encoder rows. site: RPR_CROSS_SITE_BLOCK = the block kernel's
 * launcher (training forward), _STEP = a sequential step (B = beams), _TAIL = the tail pass (B = beams x tail positions).
 * The index of the last attended key + 1 of every query is computed by the hook as a search does (into ctx scratch), so a
 * query without an attended key raises RPR_STATUS_EMPTY_QUERY and gets zeros. */
#define RPR_CROSS_SITE_BLOCK 0
#define RPR_CROSS_SITE_STEP 1
#define RPR_CROSS_SITE_TAIL 2
typedef struct rpr_cross_attn_op {
  const float* q;           /* [Q * B, H * dkv] */
  const float* xk;          /* K row (query, j) at xk + (query * Lq + j) * xld, or (offs[query] + j) * xld */
  const float* xv;
  const int32_t* mask;      /* [Q, Lq] */
  const int32_t* offs;      /* nullable (packed encoder rows) */
  const int32_t* nq_dev;    /* nullable */
  float* out;               /* [Q * B, H * dkv] */
  void* out_planes;
  int64_t plane_stride;
  int32_t site, xld, Q, B, H, Lq, dkv;
} rpr_cross_attn_op;
int rpr_op_cross_attn(rpr_ctx* ctx, const rpr_cross_attn_op* op, int32_t* out_kernel, void* stream);
/* Self-attention of the tail pass: sequence s = entry * B + b (s < *nseq_dev) has L - T rows (positions T..L-1) in qkv;
 * positions < T come from the cache of stage query kvq[entry] (NULL: flist[entry]) through the ancestry row
 * flist[entry] * B + b, positions >= T from the sequence's own rows, causally. */
typedef struct rpr_tail_self_attn_op {
  const float* qkv;         /* [nseq_cap * (L - T), 3 * H * dkv] */
  const float* kcache;
  const float* vcache;
  const uint16_t* anc;
  const int32_t* flist;
  const int32_t* kvq;       /* nullable */
  const int32_t* nseq_dev;
  const float* rel_bias;    /* [num_buckets, H] */
  float* out;               /* [nseq_cap * (L - T), H * dkv] */
  void* out_planes;
  int64_t plane_stride, q_stride, h_stride, pos_stride, slot_stride;
  int32_t anc_ld, num_buckets, max_distance, nseq_cap, B, H, T, L, dkv;
} rpr_tail_self_attn_op;
int rpr_op_tail_self_attn(rpr_ctx* ctx, const rpr_tail_self_attn_op* op, int32_t* out_kernel, void* stream);
/* ---- attention test hooks of the training step: the backward of both attention sites and their forward with dropped-out
 * probabilities, each through the site's own planner (plan_train_*) and launcher, reported and refused as above. fp32 only.
 * The dropout of the probabilities is the step's (DESIGN.md "Dropout in the training step"): the key is built from rate,
 * seed and step as rpr_set_train_dropout's is, `site` is the 16-bit site of the probabilities and L the positions per
 * sequence of the mask's coordinates (query row r of a block is position r % L of sequence block * (rows / L) + r / L;
 * self-attention: L = Ls). rate = 0: no dropout (the two backward hooks; the two drop-forward hooks refuse it). */
typedef struct rpr_attn_drop {
  uint64_t seed, step;
  float rate;               /* 0 <= rate < 1 */
  int32_t site, L;
} rpr_attn_drop;
/* Self-attention over S sequences of Ls rows (encoder: bidirectional buckets, key mask; causal: the teacher-forced decoder).
 * rpr_op_train_self_attn_bwd (launch_self_attn_bwd) reads qkv, dO and writes dqkv and dbias += the relative-bias gradient
 * (its per-(sequence, head) parts go through ctx scratch as in the step); rpr_op_train_self_attn_drop_fwd
 * (launch_self_attn_drop_fwd) reads qkv and writes out. */
typedef struct rpr_train_self_attn_op {
  const float* qkv;         /* [S * Ls, 3 * H * dkv]: q | k | v */
  const float* dO;          /* [S * Ls, H * dkv] (backward) */
  const int32_t* mask;      /* [S, Ls] key mask; NULL with causal */
  const float* rel_bias;    /* [num_buckets, H] */
  float* dqkv;              /* [S * Ls, 3 * H * dkv] (backward) */
  float* dbias;             /* [num_buckets, H], added to (backward) */
  float* out;               /* [S * Ls, H * dkv] (drop-forward) */
  rpr_attn_drop drop;
  int32_t num_buckets, max_distance, S, Ls, H, dkv, causal;
} rpr_train_self_attn_op;
int rpr_op_train_self_attn_bwd(rpr_ctx* ctx, const rpr_train_self_attn_op* op, int32_t* out_kernel, void* stream);
int rpr_op_train_self_attn_drop_fwd(rpr_ctx* ctx, const rpr_train_self_attn_op* op, int32_t* out_kernel, void* stream);
/* Cross-attention of the n = docs x L decoder rows of each of bz queries against the query's Lq encoder rows (K row
 * (query, j) at xk + (query * Lq + j) * xld, V likewise at xv). rpr_op_train_cross_attn_bwd (launch_cross_attn_bwd) reads q,
 * dO and writes dq and, in the layout of xk / xv, dxk and dxv (the head's dkv columns of every row, nothing else of the row);
 * rpr_op_train_cross_attn_drop_fwd (launch_cross_attn_drop_fwd) reads q and writes out. The key mask is required. */
typedef struct rpr_train_cross_attn_op {
  const float* q;           /* [bz * n, H * dkv] */
  const float* dO;          /* [bz * n, H * dkv] (backward) */
  const float* xk;
  const float* xv;
  const int32_t* mask;      /* [bz, Lq] */
  float* dq;                /* [bz * n, H * dkv] (backward) */
  float* dxk;               /* rows of xld floats (backward) */
  float* dxv;
  float* out;               /* [bz * n, H * dkv] (drop-forward) */
  rpr_attn_drop drop;
  int32_t xld, bz, n, Lq, H, dkv;
} rpr_train_cross_attn_op;
int rpr_op_train_cross_attn_bwd(rpr_ctx* ctx, const rpr_train_cross_attn_op* op, int32_t* out_kernel, void* stream);
int rpr_op_train_cross_attn_drop_fwd(rpr_ctx* ctx, const rpr_train_cross_attn_op* op, int32_t* out_kernel, void* stream);
/* ---- test hook of the row-wise kernels of the training step: one launcher of train_kernels.hip / dense_head.hip on the
 * caller's device buffers, through the launch_* function the step itself calls (its grid arithmetic lives there alone).
 * One flat descriptor: op selects the launcher; src / dst are [dev] pointers, dims and f the launcher's integer and float
 * arguments, all in the order listed per op below (unused entries 0 / NULL; "?" = nullable). A refused shape returns
 * RPR_ERR_INVALID and launches nothing. The hook returns after the stream has drained. Shapes: every row width (d, C) is a
 * multiple of 4 floats, as in the step.
 *   RPR_TR_RMSNORM_BWD     launch_rmsnorm_bwd. src x [rows,d], w [d], dh [rows,d], dres? [rows,d]; dst dx [rows,d],
 *                          w_part [ceil(rows/16), d], dw? [d]; dims rows, d (<= 4096), accumulate_dw; f eps, post
 *   RPR_TR_COLSUM_MULTI    launch_colsum_multi. src part_i [nparts_i, d] (i < n <= 4); dst out_i [d]; dims d, n, nparts_0..3
 *   RPR_TR_GOLD_SCORES     launch_gold_scores. src x? [S L, d] fp32, ln [d], out_embeds [L,V,d], codes? [S,L], x_planes?
 *                          ([2] f16 planes of x / 16, plane stride dims[4] elements; exactly one of x, x_planes);
 *                          dst scores? [S L], hidden? [S L, d] (exactly one; hidden: the normalised rows, no codes);
 *                          dims S, L, d, V, plane_stride; f eps, post
 *   RPR_TR_GOLD_SCORE_BWD  launch_gold_score_bwd. src x, ln, out_embeds, out_idx [rows] (rows of out_embeds, caller-checked),
 *                          dscores [rows]; dst dh [rows,d], de [rows,d]; dims rows, d; f eps, post
 *   RPR_TR_GOLD_ROWDOT     launch_gold_rowdot. src hd [rows,d], out_embeds, out_idx, dscores? (NULL: forward);
 *                          dst scores (forward), dh, de (backward); dims rows, d
 *   RPR_TR_MARGIN_MSE      launch_margin_mse. src scores [bz,2,L], teacher_pos [np,bz], teacher_neg [np,bz], prefix_lens [np];
 *                          dst losses [np], margins? [np,bz]; dims np, bz, L
 *   RPR_TR_MARGIN_MSE_BWD  launch_margin_mse_bwd. src margins [np,bz], teacher_pos, teacher_neg, prefix_lens;
 *                          dst dscores [bz,2,L]; dims np, bz, L
 *   RPR_TR_DENSE_MSE_FWD   launch_dense_mse_head_fwd. src hF [3 bz, d], teacher_pos [bz], teacher_neg [bz];
 *                          dst scores [bz,2], margins [bz], g [bz], loss [1]; dims bz, d
 *   RPR_TR_DENSE_MSE_BWD   launch_dense_mse_head_bwd. src hF, g [bz]; dst dhF [3 bz, d]; dims bz, d
 *   RPR_TR_RELU_BWD        launch_relu_bwd. src act [n]; dst dy [n] (in place); dims n (n % 4 == 0)
 *   RPR_TR_DEC_EMBED       launch_train_dec_embed. src start [d], in_embeds [L,V,d], codes [S,L]; dst out? [S L, d] fp32,
 *                          planes? ([2] f16, plane stride dims[4]; exactly one of out, planes), ssq? [S L] uint64;
 *                          dims S, L, d, V, plane_stride
 *   RPR_TR_TRAIN_INDICES   launch_train_indices. src codes [S,L]; dst in_idx [S L], out_idx [S L]; dims S, L, V
 *   RPR_TR_SCATTER_FIX     launch_scatter_rows_fix. src rows [rows,d], idx [rows] (< 0: skipped; table rows caller-checked);
 *                          dst acc (int64 [table, d], 2^-32 fixed point, added to); dims rows, d
 *   RPR_TR_FIX_FLUSH       launch_fix_flush. dst acc [n] (zeroed), table [n] fp32 (added to); dims n
 *   RPR_TR_SUM_SELECTED    launch_sum_selected_rows. src rows [rows,d], sel [rows]; dst out [d] (added to); dims rows, d
 *   RPR_TR_S2S_HEAD_FWD    launch_s2s_head_fwd. src hF [bz L, d], E [L,V,d], labels [bz L]; dst dlogits [bz L, V],
 *                          row_loss [bz L], label_lp? [bz L], loss [1]; dims bz, L, d, V (d % 32 == 0, V % 64 == 0, V <= 1024)
 *   RPR_TR_S2S_HEAD_BWD    launch_s2s_head_bwd. src hF, E, dlogits; dst dH [bz L, d], dE [L,V,d]; dims bz, L, d, V
 *   RPR_TR_ABSMAX2         launch_absmax2. src x0 [n0], x1? [n1]; dst out [2] (bit-pattern maximum with what is there:
 *                          the caller zeroes it); dims n0, n1
 *   RPR_TR_SPLIT_DYN       launch_split_dyn. src x [R, ldi], amax [1]; dst out [2][R][C] f16; dims R, C, ldi
 *   RPR_TR_SPLIT_DYN_T     launch_split_dyn_T. src x, amax; dst out_t [2][C][Rpad] f16, out_plain? [2][R][C];
 *                          dims R, C, ldi, Rpad (Rpad even, >= R)
 *   RPR_TR_TO_BF16         launch_to_bf16. src x [R, ldi]; dst out [R][C] bf16; dims R, C, ldi
 *   RPR_TR_TO_BF16_T       launch_to_bf16_T. src x, relu_act? [R, ldi]; dst out_t [C][ldt] bf16 (columns < Rpad written),
 *                          out_plain? [R][C]; dims R, C, ldi, Rpad, ldt (0 = Rpad)
 *   RPR_TR_RMSNORM_BF16_T  launch_rmsnorm_bf16_T. src x [rows,d], w [d]; dst out_plain [rows][d] bf16, out_t [d][ldt] bf16;
 *                          dims rows, d, Rpad, ldt (d <= 1024, d % 8 == 0, Rpad % 32 == 0); f eps, post
 *   RPR_TR_WEIGHTS_BF16    launch_weights_bf16. src seg_i [R_i, C_i] (i < n <= 5; R_i even, C_i % 4 == 0); dst plain, tr (bf16,
 *                          segment i at element offset sum_{j<i} R_j C_j: [R_i][C_i] and [C_i][R_i]); dims n, R_0, C_0, R_1, ...
 *   RPR_TR_TRANSPOSE_PAD   launch_transpose_pad. src in [R, ldi]; dst out [C][Rpad]; dims R, C, ldi, Rpad */
enum { RPR_TR_RMSNORM_BWD = 0, RPR_TR_COLSUM_MULTI = 1, RPR_TR_GOLD_SCORES = 2, RPR_TR_GOLD_SCORE_BWD = 3, RPR_TR_GOLD_ROWDOT = 4,
       RPR_TR_MARGIN_MSE = 5, RPR_TR_MARGIN_MSE_BWD = 6, RPR_TR_DENSE_MSE_FWD = 7, RPR_TR_DENSE_MSE_BWD = 8, RPR_TR_RELU_BWD = 9,
       RPR_TR_DEC_EMBED = 10, RPR_TR_TRAIN_INDICES = 11, RPR_TR_SCATTER_FIX = 12, RPR_TR_FIX_FLUSH = 13, RPR_TR_SUM_SELECTED = 14,
       RPR_TR_S2S_HEAD_FWD = 15, RPR_TR_S2S_HEAD_BWD = 16, RPR_TR_ABSMAX2 = 17, RPR_TR_SPLIT_DYN = 18, RPR_TR_SPLIT_DYN_T = 19,
       RPR_TR_TO_BF16 = 20, RPR_TR_TO_BF16_T = 21, RPR_TR_RMSNORM_BF16_T = 22, RPR_TR_WEIGHTS_BF16 = 23, RPR_TR_TRANSPOSE_PAD = 24,
       RPR_TR_COUNT = 25 };
typedef struct rpr_train_rows_op {
  const void* src[6];
  void* dst[6];
  int32_t op;
  int32_t dims[11];
  float f[4];
} rpr_train_rows_op;
int rpr_op_train_rows(rpr_ctx* ctx, const rpr_train_rows_op* op, void* stream);
/* Name of an AttnKernel value (csrc/attn_route.h RPR_ATTN_KERNELS), NULL when out of range. Host only. */
const char* rpr_attn_kernel_name(int kernel);
/* Number of AttnKernel values (names 0 .. n - 1). Host only. */
int rpr_attn_kernel_count(void);
/* Encoder forward only (reference generation.py:132-137): out [Q, Lq, d_model]. */
int rpr_encode(rpr_ctx* ctx, rpr_model* model, const int32_t* input_ids, const int32_t* attention_mask,
               int32_t Q, int32_t Lq, float* out, void* stream);

/* ---- residual quantization: docid creation (reference: faiss.IndexResidualQuantizer trained and applied by
 * tasks/evaluator.py:405-421 and aq_preprocess/create_customized_smtid_file.py) ----
 * Greedy residual k-means, M levels of K codewords (DESIGN.md "Residual quantization"): per level, K initial centroids
 * are rows of the level's residuals, then niter Lloyd iterations (assign = argmin_k |c_k|^2 - 2 r.c_k in fp32, smallest k
 * on ties; centroid = fp64 mean of its rows in row order, rounded to fp32 once; a centroid without rows keeps its value),
 * then a last assignment and r -= c_m[code]. Deterministic: no float atomics, two runs are bit-identical.
 * d % 32 == 0, K % 64 == 0, 64 <= K <= 1024, 1 <= n <= 2^30; anything else is RPR_ERR_INVALID. */
/* x:          [dev] fp32 [n, d] training rows (the caller samples them; n >= K); not modified
 * init_idx:   [host] int32 [M, K] initial centroid rows of every level, indices into the level's residual rows
 * codebooks:  [dev] fp32 [M, K, d] out
 * level_mse:  [host] fp64 [M] or NULL: mean |r|^2 of the training rows after level m (synchronises the stream) */
int rpr_rq_train(rpr_ctx* ctx, const float* x, int64_t n, int32_t d, int32_t M, int32_t K, int32_t niter,
                 const int32_t* init_idx, float* codebooks, double* level_mse, void* stream);
/* Encodes one device chunk with trained codebooks: codes [dev] uint16 [n, M]; level_sse [host] fp64 [M] or NULL: sum of
 * |r|^2 over the chunk's rows after level m (synchronises the stream). x is not modified (the residuals live in the ctx
 * workspace: n * d * 4 bytes); larger inputs are streamed chunk by chunk by the caller, the codes do not depend on the
 * chunking. */
int rpr_rq_encode(rpr_ctx* ctx, const float* x, int64_t n, int32_t d, const float* codebooks, int32_t M, int32_t K,
                  uint16_t* codes, double* level_sse, void* stream);
/* The same with a beam (faiss's max_beam_size; DESIGN.md 9c, tests/rq_beam_ref.py restates it in numpy). A row keeps up to
 * `beam` candidate encodings: b_0 = 1 (the row), b_{m+1} = min(beam, b_m K). At level m every candidate (s, k), s < b_m,
 * k < K, has total(s, k) = |r_s|^2 + (|c_k|^2 - 2 r_s.c_k): the score in fp32 as in rpr_rq_encode, |r_s|^2 a fixed-order
 * sum over the stored fp32 residual, the two added in fp64. The b_{m+1} smallest totals form the next beam, exact ties to
 * the smaller parent slot s, then the smaller k, stored in that order (slot 0 is the best; nothing is de-duplicated);
 * residual = fp32(r_s - c_k). codes[n, M] is the history of slot 0 after the last level, level_sse[m] the sum of slot 0's
 * |r|^2 after level m. beam = 1 is rpr_rq_encode: the same codes and the same level_sse bits. Deterministic, no float
 * atomics; a row's codes do not depend on the chunking. Inputs must be finite. The limits of rpr_rq_encode and
 * 1 <= beam <= 8; anything else is RPR_ERR_INVALID. Workspace in the context, B = beam:
 *   2 * n * B * d * 4   two residual planes (a parent is read by several children: a level cannot run in place)
 * + n * B * 8           |r|^2 of the entries, two planes
 * + n * B * B * 6       a level's candidates: the B best (score fp32, code u16) of every entry
 * + M * n * B * 3       parent slot (u8) and code (u16) of every entry of every level
 * + M * K * 4 + M * ceil(n / 128) * 8   codeword norms and per-block fp64 partials, as rpr_rq_encode. */
int rpr_rq_encode_beam(rpr_ctx* ctx, const float* x, int64_t n, int32_t d, const float* codebooks, int32_t M, int32_t K,
                       int32_t beam, uint16_t* codes, double* level_sse, void* stream);

/* ---- searching the residual-quantizer index (reference --task=aq_evaluate: evaluate.py:302-332,
 * AddictvieQuantizeIndexer.search, tasks/evaluator.py:423-443) ---- */
/* Dense embedding of a text: encoder, then ONE decoder position fed with the start embedding (decoder_input_ids = [-1]);
 * out [dev] fp32 [bz, d_model] = decoder_last_hidden_state[:, 0, :] after the final RMSNorm and the scaleup_output_hidden
 * factor (T5SeqAQEncoder.query_encode / T5AQEncoder.query_encode, modeling/t5_generative_retriever.py:786-792, 891-897).
 * The pass is rpr_lngknp_forward's with n_docs = 1, L = 1 and follows the context's precision like it. input_ids /
 * attention_mask: [dev] int32 [bz, Lq]; Lq <= 256; d_kv 64 or 128. */
int rpr_embed(rpr_ctx* ctx, rpr_model* model, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz,
              int32_t Lq, float* out, void* stream);
/* Top-k inner-product search over the codes rpr_rq_encode wrote (faiss.IndexResidualQuantizer.search with
 * METRIC_INNER_PRODUCT). Exact semantics (tests/rq_search_ref.py restates them in numpy):
 *   LUT[q][m][k]  = <queries[q], codebooks[m][k]> from the exact-fp32 MFMA GEMM (one fixed fp32 chain per entry);
 *   score[q][n]   = ((LUT[q][0][c_n0] + LUT[q][1][c_n1]) + ...) in fp32, levels in ascending order: the inner product
 *                   with the decoded vector;
 *   ranking       = score descending, exact ties to the smaller row n; -0.0 equals +0.0 (and is returned as +0.0);
 *   topk > N      : the tail of a row is idx = -1, score = -inf (faiss's convention).
 * Inputs must be finite. Codes must be < K; a larger value is clamped to K - 1 (nothing outside the LUT is read).
 * Deterministic: two runs are bit-identical, no result depends on the order in which atomics land, and the rows of a
 * query do not depend on how the queries are batched. All pointers are device pointers:
 *   queries [Q, d] fp32, codebooks [M, K, d] fp32, codes [N, M] uint16, out_idx [Q, topk] int64, out_scores [Q, topk] fp32.
 * d % 32 == 0, K % 64 == 0, 64 <= K <= 1024, 1 <= M <= 64, 1 <= N <= 2^31 - 1, 1 <= topk <= 2048, Q >= 1 (large Q is
 * chunked inside); anything else is RPR_ERR_INVALID. Device scratch beyond the caller's buffers stays under 64 MB (the
 * Q x N scores are never stored: the selection recomputes them pass by pass). */
int rpr_rq_search(rpr_ctx* ctx, const float* queries, int32_t Q, int32_t d, const float* codebooks, int32_t M, int32_t K,
                  const uint16_t* codes, int64_t N, int32_t topk, int64_t* out_idx, float* out_scores, void* stream);

/* ---- exact dense retrieval (reference --task=retrieve: faiss.IndexFlatIP.search over the collection's embeddings) ---- */
/* Exact top-k inner-product search over a block of the fp32 embedding matrix. x is rows row_base .. row_base + n - 1 of the
 * collection, row-major [n, d]. Exact semantics (tests/flat_search_ref.py restates them in numpy):
 *   score[q][r]   = <queries[q], x[r]> from the exact-fp32 MFMA GEMM: one fixed fp32 chain per entry, whatever
 *                   rpr_set_precision says, whatever the query batch and however the rows are cut into blocks;
 *   ranking       = score descending, exact ties to the smaller GLOBAL row; -0.0 equals +0.0 (and is returned as +0.0);
 *   merge == 0    : io_idx / io_scores [Q, topk] receive the top topk of this block; missing entries are idx = -1,
 *                   score = -inf;
 *   merge == 1    : the top topk of the union of this block and the entries already in io_* (a previous result: sorted,
 *                   the idx < 0 entries last, which are ignored). The caller guarantees that the stored rows are not rows
 *                   of this block.
 * Searching [0, N) in one call therefore equals chaining any partition of it through merge, in any order, bit for bit.
 * Inputs must be finite. Deterministic: no float atomics, two runs are bit-identical. All pointers are device pointers:
 *   queries [Q, d] fp32, x [n, d] fp32, io_idx [Q, topk] int64, io_scores [Q, topk] fp32.
 * d % 32 == 0, d >= 32, Q >= 1, n >= 1, row_base >= 0, row_base + n <= 2^31 - 1, 1 <= topk <= 2048, merge 0 or 1; anything
 * else is RPR_ERR_INVALID. The Q x n scores never exist in full: the rows are walked in sub-blocks so that the score
 * scratch stays within 256 MB (csrc/common.h FLAT_SCRATCH_BYTES), large Q is chunked as in rpr_rq_search; the scratch
 * lives in the context's workspace. */
int rpr_flat_search(rpr_ctx* ctx, const float* queries, int32_t Q, int32_t d, const float* x, int64_t n, int64_t row_base,
                    int32_t topk, int64_t* io_idx, float* io_scores, int32_t merge, void* stream);

/* ---- cross-encoder teacher (reference modeling/cross_encoder.py: HF BertForSequenceClassification, one logit) ---- */
/* A post-LayerNorm BERT encoder with absolute positions, erf GELU, the tanh pooler and a [1, hidden] classifier, run over a
 * PACKED batch: only attended tokens exist as rows. By default everything is fp32: the products are the
 * exact-fp32 MFMA GEMM whatever rpr_set_precision says (rpr_xenc_set_precision below switches one model to f16 operands).
 * All weight pointers are device pointers owned by the caller, which keeps
 * them alive while the handle lives; nn.Linear layout [out, in]. The per-layer tensors are stacked: layer l of qkv_w is
 * qkv_w + l * 3 * hidden * hidden (rows: query, then key, then value), of ff1_w is ff1_w + l * d_ff * hidden, and so on. */
typedef struct rpr_xenc_desc {
  int32_t vocab_size, hidden, layers, heads, d_ff, max_pos, type_vocab;
  float ln_eps;
  const float *word_emb, *pos_emb, *type_emb, *emb_ln_w, *emb_ln_b;
  const float *qkv_w, *qkv_b, *ao_w, *ao_b, *ln1_w, *ln1_b, *ff1_w, *ff1_b, *ff2_w, *ff2_b, *ln2_w, *ln2_b;
  const float *pool_w, *pool_b, *cls_w, *cls_b;
} rpr_xenc_desc;
typedef struct rpr_xenc rpr_xenc;

/* Binds the weights (nothing is copied). RPR_ERR_INVALID: a NULL pointer, a dimension below 1, hidden % heads != 0. */
int rpr_xenc_load(rpr_ctx* ctx, const rpr_xenc_desc* desc, rpr_xenc** out);
void rpr_xenc_free(rpr_xenc* model);
/* One logit per sequence. T = seq_off[bz] rows:
 *   input_ids, token_type_ids, position_ids: [dev] int32 [T], the attended tokens of sequence 0, then of sequence 1, ...;
 *       position_ids are the tokens' ORIGINAL positions (they differ from 0, 1, 2, ... where the mask had a hole). The
 *       caller guarantees ids inside their tables (the kernel clamps them: memory safety, not semantics);
 *   seq_off: [HOST] int32 [bz + 1], seq_off[0] = 0, non-decreasing: sequence b owns rows seq_off[b] .. seq_off[b + 1] - 1.
 *       Read before the call returns;
 *   out_scores: [dev] fp32 [bz]: classifier(tanh(pooler(first row of the sequence))).
 * Asynchronous on `stream`; no host synchronisation once the workspaces are warm. They live in the context and grow on
 * demand: a call with more rows than any before frees and reallocates them (hipFree synchronises the device) and drops
 * the context's captured search graphs, like every other entry point that sizes a workspace. Deterministic: no atomics,
 * the same call twice gives the same bits (another batch composition may pick another GEMM tile: last-bit differences).
 * RPR_ERR_INVALID, before anything is enqueued: a head size other than 32 or 64, hidden % 32 or d_ff % 32 nonzero,
 * hidden > 4096, bz < 1 or bz > 2^20, seq_off[0] != 0, an empty sequence, a sequence longer than min(max_pos, 512).
 * RPR_ERR_OOM: no host memory for the tile list. */
int rpr_xenc_score(rpr_ctx* ctx, rpr_xenc* model, const int32_t* input_ids, const int32_t* token_type_ids,
                   const int32_t* position_ids, const int32_t* seq_off, int32_t bz, float* out_scores, void* stream);
/* Precision of one model's rpr_xenc_score calls (a new model is RPR_XENC_F32).
 *   RPR_XENC_F32: fp32 throughout, as described above.
 *   RPR_XENC_F16: the arithmetic of torch's fp16 autocast, how the reference runs its teacher: the four products of a layer
 *       and both attention products take f16 operands (round to nearest even) and accumulate in fp32 on the f16 matrix
 *       cores; q | k | v, the attention probabilities, the attention output and the GELU output are stored as f16; the
 *       residual stream, LayerNorm, softmax, biases, embeddings, pooler and classifier stay fp32. A stored value beyond
 *       +-65504 becomes +-inf and the pair's score non-finite, as under autocast: check the scores with isfinite.
 *       Same limits, determinism and workspace rules as the fp32 mode.
 * The first switch to RPR_XENC_F16 makes f16 copies of qkv_w, ao_w, ff1_w and ff2_w on `stream` (owned by the model, freed
 * by rpr_xenc_free; the fp32 weights must not change afterwards). Switching back keeps the copies and restores the fp32
 * bits. Any other value: RPR_ERR_INVALID, nothing changes. RPR_ERR_OOM: no device memory for the copies. */
#define RPR_XENC_F32 0
#define RPR_XENC_F16 1
int rpr_xenc_set_precision(rpr_ctx* ctx, rpr_xenc* model, int precision, void* stream);
int rpr_xenc_get_precision(const rpr_xenc* model);

#ifdef __cplusplus
}
#endif
#endif /* RIPOR_HIP_H */
