// C-ABI of libripor_hip.so (see include/ripor_hip.h): context, model binding, trie, test hooks, profiling, and the
// driver of one constrained beam search: its plan (search_plan.h), workspace, the two lanes of a large batch, and the capture of
// what passes.hip enqueues (T5 encoder once + L KV-cached decoder steps, each fused with the trie mask / top-B / beam
// expand) on one HIP stream, replayed as a hipGraph (no host synchronisation inside the search; the reference syncs
// >= 1 + 2*B*Q times per step).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <tuple>
#include <vector>

#include "internal.h"

namespace rpr {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int hip_fail(hipError_t e, const char* what, const char* file, int line) {
  g_err = std::string("HIP error ") + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ") in " + what + " at " +
          file + ":" + std::to_string(line);
  (void)hipGetLastError();
  return e == hipErrorOutOfMemory ? RPR_ERR_OOM : RPR_ERR_HIP;
}

// HF T5Attention._relative_position_bucket in float32 (log in float32, truncation toward zero);
// rel = key_pos - query_pos. Pinned against the torch expression in tests/test_host_logic.py.
int rel_bucket(int rel, int bidirectional, int num_buckets, int max_distance) {
  int bucket = 0, n;
  if (bidirectional) {
    num_buckets /= 2;
    if (rel > 0) bucket += num_buckets;
    n = rel < 0 ? -rel : rel;
  } else {
    n = rel < 0 ? -rel : 0;
  }
  const int max_exact = num_buckets / 2;
  if (n < max_exact) return bucket + n;
  const float v = logf((float)n / (float)max_exact) / (float)log((double)max_distance / (double)max_exact) *
                  (float)(num_buckets - max_exact);
  int large = max_exact + (int)v;
  if (large > num_buckets - 1) large = num_buckets - 1;
  return bucket + large;
}

// The bucket tables the attention kernels index, as device arrays the caller owns (hipFree): enc [2 MAX_LQ - 1], bucket of
// rel = key - query at rel + MAX_LQ - 1 (bidirectional); dec [MAX_DEC_LEN], bucket of rel = -n (unidirectional). One place
// for a model's tables (rpr_load_model_ext) and the attention test hooks (rpr_op_*_attn). Either output may be null.
int make_bucket_tables(int num_buckets, int max_distance, int32_t** enc, int32_t** dec) {
  std::vector<int32_t> eb(2 * MAX_LQ - 1), db(MAX_DEC_LEN);
  for (int rel = -(MAX_LQ - 1); rel <= MAX_LQ - 1; ++rel) eb[rel + MAX_LQ - 1] = rel_bucket(rel, 1, num_buckets, max_distance);
  for (int n = 0; n < MAX_DEC_LEN; ++n) db[n] = rel_bucket(-n, 0, num_buckets, max_distance);
  if (enc) {
    RPR_HIP(hipMalloc(enc, eb.size() * 4));
    RPR_HIP(hipMemcpy(*enc, eb.data(), eb.size() * 4, hipMemcpyHostToDevice));
  }
  if (dec) {
    RPR_HIP(hipMalloc(dec, db.size() * 4));
    RPR_HIP(hipMemcpy(*dec, db.data(), db.size() * 4, hipMemcpyHostToDevice));
  }
  return RPR_OK;
}

// |logit| <= sqrt(d_model) * max_row |E_out[r] * ln_final| * scaleup factor for ANY decoder state (Cauchy-Schwarz on the
// RMS-normalised hidden state): the bound behind the forced-tail fork's masked-candidate proof (passes.hip: enqueue_fork).
int compute_logit_bound(rpr_ctx* c, rpr_model* m, hipStream_t s, float* out) {
  const auto& d = m->d;
  float* slot = reinterpret_cast<float*>(c->status + 9);   // device word next to the weight-range probe
  RPR_HIP(hipMemsetAsync(slot, 0, 4, s));
  RPR_HIP(launch_max_row_norm(d.out_embeds, d.dec_final_ln, d.L * d.V, d.d_model, slot, s));
  float mx = 0.f;
  RPR_HIP(hipMemcpyAsync(&mx, slot, 4, hipMemcpyDeviceToHost, s));
  RPR_HIP(hipStreamSynchronize(s));
  const float post = d.scaleup_output_hidden ? (float)pow((double)d.d_model, -0.5) : 1.0f;
  *out = 1.001f * mx * sqrtf((float)d.d_model) * post + 1.0f;   // slack for the split-precision arithmetic
  return RPR_OK;
}

int refresh_weight_planes(rpr_ctx* c, rpr_model* m, hipStream_t s) {
  // the weight-range probe has its own device word (status[8]): the ctx's sticky flags (status[0..3]) may hold something
  // nobody has read yet — searches on another model, a forward enqueued before the optimizer step
  unsigned int* probe = c->status + 8;
  RPR_HIP(hipMemsetAsync(probe, 0, 4, s));
  for (const auto& j : m->plane_jobs)
    RPR_HIP(launch_split_planes(j.w, j.dst, j.n, j.plane_stride ? j.plane_stride : j.n, s, W_PLANE_SCALE * j.pre, j.ln, m->d.d_model, probe));
  unsigned int sat = 0;
  RPR_HIP(hipMemcpyAsync(&sat, probe, 4, hipMemcpyDeviceToHost, s));
  RPR_HIP(hipStreamSynchronize(s));
  m->f32_only = sat != 0;
  m->l0_valid = false;   // the layer-0 Q/K/V table is made from in_embeds and these planes: the next search makes it again
  // the weights changed (optimizer step, or a caller writing through rpr_param_info's pointers): the logit bound of the
  // forced-tail proof follows them, and so do the graphs that hold the spread limit derived from it by value
  float lb = m->logit_bound;
  const int e = compute_logit_bound(c, m, s, &lb);
  if (e) return e;
  if (lb != m->logit_bound) {
    m->logit_bound = lb;
    drop_graphs(c, [m](const GraphKey& k) { return k.m == m; });
  }
  return RPR_OK;
}

}  // namespace rpr

using namespace rpr;

namespace {

// Precision of what one call enqueues (effective_precision, or the plan's), restored on every return path
struct PrecGuard {
  rpr_ctx* c; int saved;
  PrecGuard(rpr_ctx* c_, int prec) : c(c_), saved(c_->precision) { c->precision = prec; }
  PrecGuard(rpr_ctx* c_, const rpr_model* m) : PrecGuard(c_, effective_precision(c_->precision, m && m->f32_only)) {}
  ~PrecGuard() { c->precision = saved; }
};

int flush_profile(rpr_ctx* c) {
  std::map<const int*, int> live;   // device counters of the pass, read once each after the events have completed
  for (auto& r : c->recs) {
    RPR_HIP(hipEventSynchronize(r.b));
    float ms = 0.f;
    RPR_HIP(hipEventElapsedTime(&ms, r.a, r.b));
    double scale = 1.0;
    if (r.live_dev && r.live_static > 0) {
      auto it = live.find(r.live_dev);
      if (it == live.end()) {
        int n = r.live_static;
        RPR_HIP(hipMemcpy(&n, r.live_dev, sizeof(int), hipMemcpyDeviceToHost));
        it = live.emplace(r.live_dev, n).first;
      }
      scale = (double)std::min(std::max(it->second, 0), r.live_static) / (double)r.live_static;
    }
    auto& d = c->done[r.cls];
    d.total_ms += ms; d.launches += 1; d.flops += r.flops * scale; d.bytes += r.bytes * scale;
    c->pool.push_back(r.a); c->pool.push_back(r.b);
  }
  c->recs.clear();
  return 0;
}

}  // namespace

extern "C" {

int rpr_abi_version(void) { return 5; }
const char* rpr_last_error(void) { return g_err.c_str(); }

int rpr_rel_bucket(int rel, int bidirectional, int num_buckets, int max_distance) {
  return rel_bucket(rel, bidirectional, num_buckets, max_distance);
}

int rpr_init(int device, rpr_ctx** out_ctx) {
  RPR_REQUIRE(out_ctx != nullptr, "out_ctx is NULL");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
    (void)hipGetLastError();
    set_error("no HIP device visible: libripor_hip.so has no CPU fallback");
    return RPR_ERR_NO_DEVICE;
  }
  RPR_REQUIRE(device >= 0 && device < n, "device index out of range");
  RPR_HIP(hipSetDevice(device));
  RPR_HIP(init_t5_kernel_attributes());
  RPR_HIP(init_beam_kernel_attributes());
  RPR_HIP(init_train_kernel_attributes());
  RPR_HIP(init_tail_kernel_attributes());
  RPR_HIP(init_attn_mfma_attributes());
  auto* c = new rpr_ctx();
  c->device = device;
  if (const char* e = getenv("RPR_PRECISION"))
    c->precision = (std::string(e) == "f32") ? RPR_PREC_F32 : (std::string(e) == "bf16") ? RPR_PREC_BF16 : RPR_PREC_F16X2;
  if (const char* e = getenv("RPR_LANE_MIN_ROWS")) c->lane_min_rows = atoi(e) > 0 ? atoi(e) : 0;
  if (const char* e = getenv("RPR_FORCED_TAIL")) c->forced_tail = atoi(e) < 0 ? 0 : (atoi(e) > 2 ? 2 : atoi(e));
  if (const char* e = getenv("RPR_FORK_DEPTHS")) {   // "4,6": explicit fork depths; "" or "0": none
    c->n_fork_override = 0;
    for (const char* p = e; *p && c->n_fork_override < MAX_FORKS;) {
      const int v = atoi(p);
      if (v > 0) c->fork_override[c->n_fork_override++] = v;
      while (*p && *p != ',') ++p;
      if (*p == ',') ++p;
    }
  }
  std::memset(c->done, 0, sizeof(c->done));
  hipError_t e = hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&c->status), 256);
  if (e == hipSuccess) e = hipMemset(c->status, 0, 256);
  if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&c->status_host), 64, hipHostMallocDefault);
  if (e != hipSuccess) {
    if (c->status) (void)hipFree(c->status);
    if (c->cap_stream) (void)hipStreamDestroy(c->cap_stream);
    delete c;
    return hip_fail(e, "ctx setup", __FILE__, __LINE__);
  }
  *out_ctx = c;
  return RPR_OK;
}

void rpr_free_ctx(rpr_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  drop_graphs(c, [](const GraphKey&) { return true; });
  auto free_ws = [](Workspace& w) {   // a Workspace is nothing but DevBufs (static_assert in internal.h)
    DevBuf* all = reinterpret_cast<DevBuf*>(&w);
    for (size_t i = 0; i < sizeof(Workspace) / sizeof(DevBuf); ++i) if (all[i].p) (void)hipFree(all[i].p);
  };
  free_ws(c->ws);
  for (Lane& ln : c->lanes) {
    free_ws(ln.ws);
    if (ln.done) (void)hipEventDestroy(ln.done);
    if (ln.stream) (void)hipStreamDestroy(ln.stream);
  }
  if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
  free_train_ws(c);
  if (c->status) (void)hipFree(c->status);
  if (c->status_host) (void)hipHostFree(c->status_host);
  for (auto& r : c->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
  for (auto e : c->pool) (void)hipEventDestroy(e);
  if (c->cap_stream) (void)hipStreamDestroy(c->cap_stream);
  delete c;
}

int64_t rpr_workspace_bytes(const rpr_ctx* c) { return c ? (int64_t)c->ws_bytes : 0; }

int rpr_set_precision(rpr_ctx* c, int precision) {
  RPR_REQUIRE(c, "NULL ctx");
  RPR_REQUIRE(precision == RPR_PREC_F32 || precision == RPR_PREC_F16X2 || precision == RPR_PREC_BF16, "unknown precision");
  c->precision = precision;
  ++c->l0_epoch;   // a precision switch drops every model's layer-0 Q/K/V table: the next split-precision search makes it again
  return RPR_OK;
}
int rpr_get_precision(const rpr_ctx* c) { return c ? c->precision : -1; }

int rpr_load_model(rpr_ctx* c, const rpr_model_desc* d, rpr_model** out) { return rpr_load_model_ext(c, d, nullptr, out); }

int rpr_load_model_ext(rpr_ctx* c, const rpr_model_desc* d, const rpr_model_ext* ext, rpr_model** out) {
  RPR_REQUIRE(c && d && out, "NULL argument");
  RPR_REQUIRE(!ext || ext->size >= (int32_t)sizeof(rpr_model_ext), "rpr_model_ext.size is smaller than the struct");
  const int ff_kind = ext ? ext->ff_kind : RPR_FF_RELU;
  RPR_REQUIRE(ff_kind == RPR_FF_RELU || ff_kind == RPR_FF_GATED_GELU, "ff_kind must be 0 (ReLU) or 1 (gated GELU)");
  RPR_REQUIRE(d->d_kv == DKV || d->d_kv == 128, "d_kv must be 64 (t5-base / t5-large) or 128 (t5-3b)");
  RPR_REQUIRE(d->d_model % 32 == 0 && d->d_ff % 32 == 0, "d_model and d_ff must be multiples of 32");
  RPR_REQUIRE(d->V >= 2 && d->V <= 65536, "decoder vocab size out of range (2..65536)");
  RPR_REQUIRE(d->L >= 1 && d->L <= MAX_DEC_LEN, "decoder length out of range");
  RPR_REQUIRE(d->rel_buckets >= 2 && d->rel_buckets <= 64, "relative_attention_num_buckets out of range");
  RPR_REQUIRE(d->num_layers >= 1 && d->num_decoder_layers >= 1 && d->num_heads >= 1, "bad layer/head count");
  RPR_REQUIRE(d->shared && d->enc_rel_bias && d->dec_rel_bias && d->enc_final_ln && d->dec_final_ln &&
                  d->start_embed && d->in_embeds && d->out_embeds && d->dec_xkv, "NULL weight pointer");
  RPR_HIP(hipSetDevice(c->device));
  auto m = std::make_unique<rpr_model>(c, *d, ff_kind);
  RPR_REQUIRE(m->params.fill(*d), "NULL per-layer weight pointer");
  // the desc's host arrays need not outlive this call
  for (int kind = K_ENC_LAYER; kind < K_END; ++kind) m->d.*layer_field(kind) = nullptr;
  if (const int e = make_bucket_tables(d->rel_buckets, d->rel_max_distance, &m->enc_bucket, &m->dec_bucket)) return e;
  // hi/lo f16 planes of every GEMM weight for the split-precision kernels
  {
    const size_t dm = d->d_model;
    int err = 0;
    unsigned int* probe = c->status + 8;   // weight-range probe word, apart from the sticky flags (refresh_weight_planes)
    RPR_HIP(hipMemset(probe, 0, 4));
    // ln (nullable): layer-norm weight folded into the columns (length = the projection's input dim, always d_model);
    // pre = extra scalar on the weights (scaleup_output_hidden on the codebooks)
    auto mk = [&](const float* wf, size_t n, __half** outp, const float* ln = nullptr, float pre = 1.0f) {
      if (err) return;
      void* p = nullptr;
      hipError_t e = hipMalloc(&p, n * 2 * sizeof(__half));
      if (e == hipSuccess) {
        m->owned.push_back(p);
        m->plane_jobs.push_back({wf, n, (__half*)p, ln, pre, 0});
        e = launch_split_planes(wf, (__half*)p, n, n, nullptr, W_PLANE_SCALE * pre, ln, (int)dm, probe);
      }
      if (e != hipSuccess) { err = hip_fail(e, "weight split", __FILE__, __LINE__); return; }
      *outp = (__half*)p;
    };
    // W_in and W_out of every sub-block of every layer: W_in carries the ln of its own sub-block (ParamOrder::weight)
    const auto& slots = m->params.slots;
    for (int dec = 0; dec < 2; ++dec)
      for (int i = 0; i < m->params.stack[dec].layers; ++i)
        for (int j = 0; j < m->params.stack[dec].nsub; ++j)
          for (int role = P_WIN; role <= P_WOUT; ++role) {
            const WeightRef r = m->params.weight(dec, i, j, role);
            mk(slots[r.slot].ptr, slots[r.slot].numel, &m->planes[r.slot], r.fold < 0 ? nullptr : slots[r.fold].ptr);
          }
    mk(d->dec_xkv, m->params.at(K_XKV).numel, &m->h_dec_xkv);
    if (!err) {   // the output codebooks, each padded to Vp rows (zero rows: their logits are 0 and never selectable)
      const size_t Vp = (size_t)m->Vp(), ps = (size_t)d->L * Vp * dm, n = (size_t)d->V * dm;
      const float pre = d->scaleup_output_hidden ? (float)pow((double)dm, -0.5) : 1.0f;
      void* p = nullptr;
      hipError_t e = hipMalloc(&p, ps * 2 * sizeof(__half));
      if (e == hipSuccess) { m->owned.push_back(p); e = hipMemset(p, 0, ps * 2 * sizeof(__half)); }
      for (int l = 0; l < d->L && e == hipSuccess; ++l) {
        __half* dst = (__half*)p + (size_t)l * Vp * dm;
        m->plane_jobs.push_back({d->out_embeds + (size_t)l * n, n, dst, d->dec_final_ln, pre, ps});
        e = launch_split_planes(d->out_embeds + (size_t)l * n, dst, n, ps, nullptr, W_PLANE_SCALE * pre, d->dec_final_ln, (int)dm, probe);
      }
      if (e != hipSuccess) err = hip_fail(e, "codebook split", __FILE__, __LINE__);
      m->h_out_embeds = (__half*)p;
    }
    if (!err) { hipError_t e = hipDeviceSynchronize(); if (e != hipSuccess) err = hip_fail(e, "sync", __FILE__, __LINE__); }
    if (err) return err;
    // a weight (times its folded layer-norm weight, times 2^8) outside the f16 range cannot be carried by the planes:
    // the model is pinned to the exact-fp32 kernels instead of being clipped silently
    unsigned int sat = 0;
    RPR_HIP(hipMemcpy(&sat, probe, 4, hipMemcpyDeviceToHost));
    if (sat) m->f32_only = true;
  }
  {  // bound of |logit| (forced-tail fork, see internal.h)
    const int e = compute_logit_bound(c, m.get(), nullptr, &m->logit_bound);
    if (e) return e;
  }
  *out = m.release();
  return RPR_OK;
}

void rpr_free_model(rpr_model* m) {
  if (!m) return;
  (void)hipSetDevice(m->ctx->device);
  (void)hipDeviceSynchronize();
  drop_graphs(m->ctx, [m](const GraphKey& k) { return k.m == m; });   // graphs that reference this model's tables
  train_forget_model(m->ctx, m);
  delete m;
}

// child arrays of the trie for its current vocab size (see rpr_trie / trie.h ChildLevels): built on the host in one pass over
// the sorted rows, uploaded once; rpr_trie_set_vocab rebuilds them (the dense tables are indexed with V)
static int upload_levels(rpr_trie* t) {
  t->free_levels();
  static const bool levels_on = [] { const char* e = getenv("RPR_SELECT_LEVELS"); return !(e && atoi(e) == 0); }();
  if (!levels_on || t->N >= ((int64_t)1 << 31) - 1) return RPR_OK;
  ChildLevels cl;
  // at most two entries per doc over all the deep levels: 8.8 M x 32 MS MARCO codes need 6.9 M (level 2 only)
  build_child_levels(t->host_sorted.data(), t->N, t->L, t->V, TRIE_NARROW, TRIE_MAX_DEEP, 2 * t->N + 1024, cl);
  auto up = [](auto*& dst, const auto& v) -> hipError_t {
    if (v.empty()) return hipSuccess;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&dst), v.size() * sizeof(v[0]));
    if (e != hipSuccess) return e;
    return hipMemcpy(dst, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice);
  };
  RPR_HIP(up(t->lvl0, cl.lvl0));
  RPR_HIP(up(t->lvl1, cl.lvl1));
  if (!cl.deep.empty()) RPR_HIP(up(t->idx2, cl.idx2));
  for (size_t i = 0; i < cl.deep.size() && i < (size_t)TRIE_MAX_DEEP; ++i) {
    RPR_HIP(up(t->d_start[i], cl.deep[i].start));
    RPR_HIP(up(t->d_tok[i], cl.deep[i].tok));
    t->d_n[i] = (int)cl.deep[i].start.size();
    t->n_deep = (int)i + 1;
  }
  t->lvl_V = t->V;
  return RPR_OK;
}

static int upload_trie(rpr_ctx* c, std::unique_ptr<rpr_trie>& t) {
  RPR_HIP(hipSetDevice(c->device));
  RPR_HIP(hipMalloc(&t->codes, t->host_sorted.size() * sizeof(uint16_t)));
  RPR_HIP(hipMemcpy(t->codes, t->host_sorted.data(), t->host_sorted.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  return upload_levels(t.get());
}

int rpr_build_trie(rpr_ctx* c, const uint16_t* codes, int64_t N, int32_t L, int32_t V, rpr_trie** out) {
  RPR_REQUIRE(c && codes && out, "NULL argument");
  RPR_REQUIRE(N > 0 && N < ((int64_t)1 << 31) - 1, "N out of range");
  RPR_REQUIRE(L >= 1 && L <= 4096 && V >= 1 && V <= 65536, "L or V out of range");
  for (int64_t i = 0; i < N * L; ++i) RPR_REQUIRE(codes[i] < V, "code >= V");
  auto t = std::make_unique<rpr_trie>();
  t->ctx = c; t->N = N; t->L = L; t->V = V;
  sort_codes(codes, N, L, t->host_sorted, t->perm);
  int e = upload_trie(c, t);
  if (e) return e;
  *out = t.release();
  return RPR_OK;
}

void rpr_free_trie(rpr_trie* t) {
  if (!t) return;
  (void)hipSetDevice(t->ctx->device);
  (void)hipDeviceSynchronize();
  drop_graphs(t->ctx, [t](const GraphKey& k) { return k.t == t; });
  delete t;
}

int64_t rpr_trie_num_rows(const rpr_trie* t) { return t ? t->N : 0; }
const int64_t* rpr_trie_perm(const rpr_trie* t) { return t ? t->perm.data() : nullptr; }

int rpr_trie_save(const rpr_trie* t, const char* path) {
  RPR_REQUIRE(t && path, "NULL argument");
  if (save_trie_file(path, t->host_sorted, t->perm, t->N, t->L, t->V, t->keys, 0, 0) != 0) {
    set_error(std::string("cannot write trie file ") + path);
    return RPR_ERR_INVALID;
  }
  return RPR_OK;
}

int rpr_trie_build_file(const uint16_t* codes, int64_t N, int32_t L, int32_t V, const char* keys, int64_t key_bytes,
                        int64_t src_size, int64_t src_mtime_ns, const char* path) {
  RPR_REQUIRE(codes && path, "NULL argument");
  RPR_REQUIRE(N > 0 && N < ((int64_t)1 << 31) - 1, "N out of range");
  RPR_REQUIRE(L >= 1 && L <= 4096 && V >= 1 && V <= 65536, "L or V out of range");
  RPR_REQUIRE(key_bytes >= 0 && (key_bytes == 0 || keys), "keys missing");
  for (int64_t i = 0; i < N * L; ++i) RPR_REQUIRE(codes[i] < V, "code >= V");
  try {
    std::vector<uint16_t> sorted;
    std::vector<int64_t> perm;
    sort_codes(codes, N, L, sorted, perm);
    const std::string k = key_bytes ? std::string(keys, (size_t)key_bytes) : std::string();
    if (save_trie_file(path, sorted, perm, N, L, V, k, src_size, src_mtime_ns) != 0) {
      set_error(std::string("cannot write trie file ") + path);
      return RPR_ERR_INVALID;
    }
  } catch (const std::exception& ex) {
    set_error(std::string("rpr_trie_build_file: ") + ex.what());
    return RPR_ERR_OOM;
  }
  return RPR_OK;
}

int rpr_trie_single_frac(const uint16_t* codes, int64_t N, int32_t Lc, int32_t L, double* out_frac) {
  RPR_REQUIRE(codes && out_frac, "NULL argument");
  RPR_REQUIRE(N > 0 && N < ((int64_t)1 << 31) - 1 && Lc >= 1 && Lc <= 4096 && L >= 1 && L <= Lc, "N, Lc or L out of range");
  try {
    std::vector<uint16_t> sorted;
    std::vector<int64_t> perm;
    sort_codes(codes, N, Lc, sorted, perm);
    std::vector<double> f;
    trie_single_frac(sorted.data(), N, Lc, L, f);
    for (int t = 0; t <= L; ++t) out_frac[t] = f[(size_t)t];
  } catch (const std::exception& ex) {
    set_error(std::string("rpr_trie_single_frac: ") + ex.what());
    return RPR_ERR_OOM;
  }
  return RPR_OK;
}

int rpr_trie_extra_mean(const uint16_t* codes, int64_t N, int32_t Lc, int32_t L, double* out_mean) {
  RPR_REQUIRE(codes && out_mean, "NULL argument");
  RPR_REQUIRE(N > 0 && N < ((int64_t)1 << 31) - 1 && Lc >= 1 && Lc <= 4096 && L >= 1 && L <= Lc, "N, Lc or L out of range");
  try {
    std::vector<uint16_t> sorted;
    std::vector<int64_t> perm;
    sort_codes(codes, N, Lc, sorted, perm);
    std::vector<double> f, mu;
    trie_single_frac(sorted.data(), N, Lc, L, f, &mu);
    for (int t = 0; t <= L; ++t) out_mean[t] = mu[(size_t)t];
  } catch (const std::exception& ex) {
    set_error(std::string("rpr_trie_extra_mean: ") + ex.what());
    return RPR_ERR_OOM;
  }
  return RPR_OK;
}

int rpr_plan_forks(const double* single_frac, const double* extra_mean, int32_t Q, int32_t B, int32_t L, int32_t forced_tail,
                   int32_t tail_extras, int32_t* out_depths, int32_t* out_drop_last) {
  RPR_REQUIRE(single_frac && extra_mean && out_depths && out_drop_last, "NULL argument");
  RPR_REQUIRE(Q >= 1 && B >= 1 && L >= 1 && L < 256 && forced_tail >= 0 && forced_tail <= 2 && tail_extras >= -1, "argument out of range");
  bool drop_last = false;
  int forks[MAX_FORKS];
  const int n = plan_forks(single_frac, extra_mean, Q, B, L, forced_tail, tail_extras_budget(tail_extras, Q, B, false), tail_extras_pool(Q), forks, &drop_last);
  for (int i = 0; i < n; ++i) out_depths[i] = forks[i];
  *out_drop_last = drop_last ? 1 : 0;
  return n;
}

int rpr_trie_file_info(const char* path, int64_t* N, int32_t* L, int32_t* V, int64_t* key_bytes, int64_t* src_size,
                       int64_t* src_mtime_ns) {
  RPR_REQUIRE(path, "NULL argument");
  int64_t h[6];
  if (trie_file_info(path, h) != 0) { set_error(std::string("not a readable RPRTRIE2 file: ") + path); return RPR_ERR_INVALID; }
  if (N) *N = h[0];
  if (L) *L = (int32_t)h[1];
  if (V) *V = (int32_t)h[2];
  if (key_bytes) *key_bytes = h[3];
  if (src_size) *src_size = h[4];
  if (src_mtime_ns) *src_mtime_ns = h[5];
  return RPR_OK;
}

int rpr_trie_file_validate(const char* path) {
  RPR_REQUIRE(path, "NULL argument");
  try {
    std::vector<uint16_t> sorted; std::vector<int64_t> perm; std::string keys, err;
    int64_t N; int L, V;
    if (load_trie_file(path, sorted, perm, N, L, V, keys, err) != 0) {
      set_error(std::string("invalid trie file ") + path + ": " + err);
      return RPR_ERR_INVALID;
    }
  } catch (const std::exception& ex) {
    set_error(std::string("rpr_trie_file_validate: ") + ex.what());
    return RPR_ERR_OOM;
  }
  return RPR_OK;
}

int rpr_trie_load(rpr_ctx* c, const char* path, rpr_trie** out) {
  RPR_REQUIRE(c && path && out, "NULL argument");
  try {
    auto t = std::make_unique<rpr_trie>();
    t->ctx = c;
    std::string err;
    if (load_trie_file(path, t->host_sorted, t->perm, t->N, t->L, t->V, t->keys, err) != 0) {
      set_error(std::string("cannot load trie file ") + path + ": " + err);
      return RPR_ERR_INVALID;
    }
    int e = upload_trie(c, t);
    if (e) return e;
    *out = t.release();
  } catch (const std::exception& ex) {   // nothing may cross the C ABI
    set_error(std::string("rpr_trie_load: ") + ex.what());
    return RPR_ERR_OOM;
  }
  return RPR_OK;
}

int rpr_trie_dims(const rpr_trie* t, int64_t* N, int32_t* L, int32_t* V, int64_t* key_bytes) {
  RPR_REQUIRE(t, "NULL trie");
  if (N) *N = t->N;
  if (L) *L = t->L;
  if (V) *V = t->V;
  if (key_bytes) *key_bytes = (int64_t)t->keys.size();
  return RPR_OK;
}

int rpr_trie_keys(const rpr_trie* t, char* out) {
  RPR_REQUIRE(t && out, "NULL argument");
  std::memcpy(out, t->keys.data(), t->keys.size());
  return RPR_OK;
}

int rpr_trie_set_vocab(rpr_trie* t, int32_t V) {
  RPR_REQUIRE(t, "NULL trie");
  RPR_REQUIRE(V >= 1 && V <= 65536, "V out of range");
  uint16_t mx = 0;
  for (uint16_t v : t->host_sorted) mx = v > mx ? v : mx;
  RPR_REQUIRE((int)mx < V, "a code of the trie is >= the requested vocab size");
  if (V == t->V) return RPR_OK;
  t->V = V;
  // the child arrays are indexed with the vocab size they were built for: rebuild them (searches captured against the old
  // tables are dropped with them)
  RPR_HIP(hipSetDevice(t->ctx->device));
  RPR_HIP(hipDeviceSynchronize());
  drop_graphs(t->ctx, [t](const GraphKey& k) { return k.t == t; });
  return upload_levels(t);
}

int rpr_d2s_open(const char* path, rpr_d2s** out) {
  RPR_REQUIRE(path && out, "NULL argument");
  auto h = std::make_unique<rpr_d2s>();
  std::string err;
  if (read_docid_to_smtid(path, h->codes, h->keys, h->N, h->L, err) != 0) {
    set_error("docid_to_smtid: " + err);
    return RPR_ERR_INVALID;
  }
  *out = h.release();
  return RPR_OK;
}

int rpr_d2s_dims(const rpr_d2s* h, int64_t* N, int32_t* L, int64_t* key_bytes) {
  RPR_REQUIRE(h, "NULL handle");
  if (N) *N = h->N;
  if (L) *L = h->L;
  if (key_bytes) *key_bytes = (int64_t)h->keys.size();
  return RPR_OK;
}

int rpr_d2s_copy(const rpr_d2s* h, uint16_t* codes, char* keys) {
  RPR_REQUIRE(h, "NULL handle");
  if (codes) std::memcpy(codes, h->codes.data(), h->codes.size() * sizeof(uint16_t));
  if (keys) std::memcpy(keys, h->keys.data(), h->keys.size());
  return RPR_OK;
}

void rpr_d2s_close(rpr_d2s* h) { delete h; }

int rpr_trie_mask(rpr_ctx* c, const rpr_trie* t, const int32_t* prefix, int32_t R, int32_t T, uint8_t* out_mask) {
  RPR_REQUIRE(c && t && prefix && out_mask, "NULL argument");
  RPR_REQUIRE(R >= 1 && T >= 1, "R and T must be >= 1");
  RPR_HIP(hipSetDevice(c->device));
  DevTmp dp, dm;
  RPR_HIP(dp.alloc((size_t)R * T * 4));
  RPR_HIP(dm.alloc((size_t)R * t->V));
  RPR_HIP(hipMemcpy(dp.p, prefix, (size_t)R * T * 4, hipMemcpyHostToDevice));
  RPR_HIP(launch_prefix_mask(t->codes, t->L, t->N, dp.as<int32_t>(), R, T, t->V, dm.as<uint8_t>(), nullptr));
  RPR_HIP(hipMemcpy(out_mask, dm.p, (size_t)R * t->V, hipMemcpyDeviceToHost));
  return RPR_OK;
}

}  // extern "C"

namespace {

// the two CU-masked lane streams of a ctx (created on first use)
bool ensure_lanes(rpr_ctx* c) {
  if (c->lanes_state) return c->lanes_state > 0;
  c->lanes_state = -1;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) { (void)hipGetLastError(); return false; }
  const int cus = prop.multiProcessorCount, words = (cus + 31) / 32;
  if (cus < 64 || words > 32) return false;
  c->lane_cus = cus / 2;
  for (int i = 0; i < 2; ++i) {
    uint32_t mask[32] = {0};
    for (int k = (i == 0 ? 0 : cus / 2); k < (i == 0 ? cus / 2 : cus); ++k) mask[k >> 5] |= 1u << (k & 31);
    if (hipExtStreamCreateWithCUMask(&c->lanes[i].stream, (uint32_t)words, mask) != hipSuccess ||
        hipEventCreateWithFlags(&c->lanes[i].done, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
  }
  if (hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); return false; }
  c->lanes_state = 1;
  return true;
}

// The plan of one search on one workspace (lane -1: the ctx's): the ctx's settings (its base), the model's facts and the call handed to
// plan_search, which asks for the trie's statistics when the automatic fork planner needs them (one pass over the sorted
// codes, on the first such search of that length)
// What rpr_search_prefixes asks for beyond rpr_search: the prefix lengths and where each one's beams go (device pointers)
struct PrefixOuts {
  int n = 0;
  int depths[MAX_DEPTHS] = {0, 0, 0};
  int32_t* tokens[MAX_DEPTHS]; float* scores[MAX_DEPTHS]; int64_t* lo[MAX_DEPTHS]; int64_t* hi[MAX_DEPTHS];
};

SearchPlan make_plan(rpr_ctx* c, const rpr_model* m, rpr_trie* tr, int Q, int Lq, int B, int L, unsigned flags, bool taps, bool margins,
                     int lane, const PrefixOuts* px = nullptr) {
  SearchModel f;
  f.logit_bound = m->logit_bound; f.V = m->d.V; f.f32_only = m->f32_only; f.l0_current = m->l0_ready(c);
  // the per-call debug switches of the selection / ranking kernels are part of the plan (tests flip them between calls)
  auto env_int = [](const char* n, int dflt) { const char* e = getenv(n); return e ? atoi(e) : dflt; };
  SearchCall a{Q, Lq, B, L, flags, taps, margins, lane, env_int("RPR_TAIL_RANK_REPLAY", 0), env_int("RPR_SELECT_RADIX", -1)};
  if (px) { a.n_depths = px->n; for (int i = 0; i < px->n; ++i) a.depths[i] = px->depths[i]; }
  return plan_search(*c, f, a, [&] {
    auto it = tr->single_frac.find(L);
    if (it == tr->single_frac.end()) {
      std::vector<double> sf, mu;
      trie_single_frac(tr->host_sorted.data(), tr->N, tr->L, L, sf, &mu);
      it = tr->single_frac.emplace(L, std::move(sf)).first;
      tr->extra_mean[L] = std::move(mu);
    }
    return TrieStats{it->second.data(), tr->extra_mean[L].data()};
  });
}

// a lane's workspace stands in c->ws for the scope (lane -1: the ctx's own stays)
struct WsGuard {
  rpr_ctx* c; int lane;
  WsGuard(rpr_ctx* c_, int l) : c(c_), lane(l) { if (lane >= 0) std::swap(c->ws, c->lanes[lane].ws); }
  ~WsGuard() { if (lane >= 0) std::swap(c->ws, c->lanes[lane].ws); }
};

// one planned search on stream s, in the workspace of its plan, which search_entry has sized
int search_one(rpr_ctx* c, rpr_model* m, rpr_trie* tr, const SearchPlan& plan, const int32_t* input_ids, const int32_t* attention_mask,
               int32_t* out_tokens, float* out_scores, int64_t* out_row_lo, int64_t* out_row_hi, double* out_margin,
               const rpr_debug_taps* taps, hipStream_t s, const PrefixOuts* px = nullptr) {
  WsGuard ws_guard(c, plan.lane);
  PrecGuard prec_guard(c, plan.prec);
  const int Q = plan.Q, L = plan.L;
  c->last_forks.assign(plan.forks, plan.forks + plan.n_forks);
  c->last_ws_mask |= plan.lane >= 0 ? (2 << plan.lane) : 1;
  Workspace& w = c->ws;
  const size_t T = (size_t)Q * plan.Lq, R = (size_t)Q * plan.B;
  RPR_HIP(hipMemcpyAsync(w.ids.p, input_ids, T * 4, hipMemcpyDeviceToDevice, s));
  RPR_HIP(hipMemcpyAsync(w.mask.p, attention_mask, T * 4, hipMemcpyDeviceToDevice, s));

  const bool eager = (plan.flags & RPR_FLAG_NO_GRAPH) || taps || c->profiling;
  if (eager) {
    Launcher Ln{c, s};
    enqueue_search(Ln, c, m, tr, plan, taps);
    if (Ln.err) return Ln.err;
  } else {
    const GraphKey key{m, tr, plan};
    auto it = c->graphs.find(key);
    if (it == c->graphs.end()) {
      hipGraph_t graph = nullptr;
      RPR_HIP(hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeThreadLocal));
      Launcher Ln{c, c->cap_stream};
      enqueue_search(Ln, c, m, tr, plan, nullptr);
      hipError_t ce = hipStreamEndCapture(c->cap_stream, &graph);
      if (Ln.err) { if (graph) (void)hipGraphDestroy(graph); return Ln.err; }
      if (ce != hipSuccess) return hip_fail(ce, "hipStreamEndCapture", __FILE__, __LINE__);
      hipGraphExec_t exec = nullptr;
      hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
      (void)hipGraphDestroy(graph);
      if (ie != hipSuccess) return hip_fail(ie, "hipGraphInstantiate", __FILE__, __LINE__);
      it = c->graphs.emplace(key, exec).first;
    }
    RPR_HIP(hipGraphLaunch(it->second, s));
  }
  RPR_HIP(hipMemcpyAsync(out_tokens, w.o_tokens.p, R * (size_t)L * 4, hipMemcpyDeviceToDevice, s));
  RPR_HIP(hipMemcpyAsync(out_scores, w.o_scores.p, R * 4, hipMemcpyDeviceToDevice, s));
  if (out_row_lo) RPR_HIP(hipMemcpyAsync(out_row_lo, w.o_lo.p, R * 8, hipMemcpyDeviceToDevice, s));
  if (out_row_hi) RPR_HIP(hipMemcpyAsync(out_row_hi, w.o_hi.p, R * 8, hipMemcpyDeviceToDevice, s));
  if (out_margin) RPR_HIP(hipMemcpyAsync(out_margin, w.o_margin.p, (size_t)Q * 8, hipMemcpyDeviceToDevice, s));
  for (int k = 0; px && k < plan.n_depths; ++k) {   // the plan's prefix lengths are px's, in its order
    RPR_HIP(hipMemcpyAsync(px->tokens[k], w.d_tokens[k].p, R * (size_t)plan.depths[k] * 4, hipMemcpyDeviceToDevice, s));
    RPR_HIP(hipMemcpyAsync(px->scores[k], w.d_scores[k].p, R * 4, hipMemcpyDeviceToDevice, s));
    RPR_HIP(hipMemcpyAsync(px->lo[k], w.d_lo[k].p, R * 8, hipMemcpyDeviceToDevice, s));
    RPR_HIP(hipMemcpyAsync(px->hi[k], w.d_hi[k].p, R * 8, hipMemcpyDeviceToDevice, s));
  }
  return RPR_OK;
}

// rpr_search (out_margin == nullptr), rpr_search_margins and rpr_search_prefixes (px != nullptr, checked by its entry):
// argument checks, weight planes, the plans, the lane split
int search_entry(rpr_ctx* c, rpr_model* m, rpr_trie* tr, const int32_t* input_ids, const int32_t* attention_mask,
                 int32_t Q, int32_t Lq, int32_t B, int32_t L, uint32_t flags, int32_t* out_tokens, float* out_scores,
                 int64_t* out_row_lo, int64_t* out_row_hi, double* out_margin, const rpr_debug_taps* taps, void* stream,
                 const PrefixOuts* px = nullptr) {
  RPR_REQUIRE(c && m && tr && input_ids && attention_mask && out_tokens && out_scores, "NULL argument");
  RPR_REQUIRE(m->ctx == c && tr->ctx == c, "model/trie belong to another ctx");
  RPR_REQUIRE(Q >= 1 && B >= 1 && B <= 65535, "Q or B out of range");
  RPR_REQUIRE(Lq >= 1 && Lq <= MAX_LQ, "Lq out of range (1..256)");
  RPR_REQUIRE(L >= 1 && L <= m->d.L && L <= tr->L, "L exceeds the model's decoder length or the trie depth");
  RPR_REQUIRE(tr->V == m->d.V, "trie V differs from the model's decoder vocab size");
  RPR_REQUIRE((int64_t)Q * B < ((int64_t)1 << 24), "Q*B too large");
  // the step self-attention splits its wave index (query, beam, head) by reciprocal multiplication, exact below
  // 2^32 / max(B, H) (launch_dec_self_attn): said here, not as a launch error in the middle of a capture
  RPR_REQUIRE((int64_t)Q * B * m->d.num_heads < ((int64_t)1 << 32) / std::max<int64_t>(B, m->d.num_heads),
              "Q * num_beams * num_heads too large for this beam count: search fewer queries per call");
  RPR_REQUIRE(select_fits(B, m->Vp()), "num_beams * decoder vocab size too large for the select kernel (about 1600 beams at V=256)");
  RPR_REQUIRE(!taps || m->Vp() == m->d.V, "debug taps need a decoder vocab size that is a multiple of 64");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  { const int pe = ensure_weight_planes(c, m, s); if (pe) return pe; }   // after an optimizer step
  { const int te = ensure_l0_table(c, m, s); if (te) return te; }        // first search of the model, or after the above
  c->last_ws_mask = 0;
  // Large batches: two halves on the two CU-masked lanes, side by side (see Lane). Results are those of one call: every
  // query is processed on its own rows. The caller's stream waits for both lanes.
  // (a call with prefix lengths runs on one workspace, like one with taps)
  const bool split = c->lane_min_rows > 0 && (int64_t)Q * B >= c->lane_min_rows && Q >= 2 && !taps && !px && ensure_lanes(c);
  // Every workspace of the call is planned once and sized BEFORE anything is enqueued: growing a buffer drops every cached
  // graph of the ctx (ensure()), which must not happen while the other lane's graph is in flight — and an allocation failure
  // then leaves nothing running
  const int32_t Qh[2] = {split ? (Q + 1) / 2 : Q, Q / 2};
  SearchPlan plans[2];
  for (int i = 0; i < (split ? 2 : 1); ++i) {
    plans[i] = make_plan(c, m, tr, Qh[i], Lq, B, L, flags, taps != nullptr, out_margin != nullptr, split ? i : -1, px);
    WsGuard ws_guard(c, plans[i].lane);
    const int e = alloc_workspace(c, m, plans[i]);
    if (e) return e;
  }
  if (split) {
    RPR_HIP(hipEventRecord(c->fork_ev, s));
    int32_t q0 = 0;
    for (int i = 0; i < 2; ++i) {
      Lane& ln = c->lanes[i];
      RPR_HIP(hipStreamWaitEvent(ln.stream, c->fork_ev, 0));
      const size_t r0 = (size_t)q0 * B;
      int e = search_one(c, m, tr, plans[i], input_ids + (size_t)q0 * Lq, attention_mask + (size_t)q0 * Lq, out_tokens + r0 * L,
                         out_scores + r0, out_row_lo ? out_row_lo + r0 : nullptr, out_row_hi ? out_row_hi + r0 : nullptr,
                         out_margin ? out_margin + q0 : nullptr, nullptr, ln.stream);
      if (e) {   // the other half may already be writing the caller's buffers: let it finish before reporting the error
        for (int k = 0; k < 2; ++k) (void)hipStreamSynchronize(c->lanes[k].stream);
        return e;
      }
      RPR_HIP(hipEventRecord(ln.done, ln.stream));
      q0 += Qh[i];
    }
    for (int i = 0; i < 2; ++i) RPR_HIP(hipStreamWaitEvent(s, c->lanes[i].done, 0));
    return RPR_OK;
  }
  return search_one(c, m, tr, plans[0], input_ids, attention_mask, out_tokens, out_scores, out_row_lo, out_row_hi, out_margin, taps, s, px);
}

}  // namespace

extern "C" {

int rpr_search(rpr_ctx* c, rpr_model* m, rpr_trie* tr, const int32_t* input_ids, const int32_t* attention_mask,
               int32_t Q, int32_t Lq, int32_t B, int32_t L, uint32_t flags, int32_t* out_tokens, float* out_scores,
               int64_t* out_row_lo, int64_t* out_row_hi, const rpr_debug_taps* taps, void* stream) {
  return search_entry(c, m, tr, input_ids, attention_mask, Q, Lq, B, L, flags, out_tokens, out_scores, out_row_lo, out_row_hi,
                      nullptr, taps, stream);
}

int rpr_search_margins(rpr_ctx* c, rpr_model* m, rpr_trie* tr, const int32_t* input_ids, const int32_t* attention_mask,
                       int32_t Q, int32_t Lq, int32_t B, int32_t L, uint32_t flags, int32_t* out_tokens, float* out_scores,
                       int64_t* out_row_lo, int64_t* out_row_hi, double* out_margin, const rpr_debug_taps* taps, void* stream) {
  RPR_REQUIRE(out_margin != nullptr, "out_margin is NULL");
  return search_entry(c, m, tr, input_ids, attention_mask, Q, Lq, B, L, flags, out_tokens, out_scores, out_row_lo, out_row_hi,
                      out_margin, taps, stream);
}

int rpr_search_prefixes(rpr_ctx* c, rpr_model* m, rpr_trie* tr, const int32_t* input_ids, const int32_t* attention_mask,
                        int32_t Q, int32_t Lq, int32_t B, int32_t L, uint32_t flags, int32_t* out_tokens, float* out_scores,
                        int64_t* out_row_lo, int64_t* out_row_hi, int32_t n_depths, const int32_t* depths,
                        int32_t* const* depth_tokens, float* const* depth_scores, int64_t* const* depth_row_lo,
                        int64_t* const* depth_row_hi, void* stream) {
  RPR_REQUIRE(n_depths >= 1 && n_depths <= MAX_DEPTHS, "n_depths out of range (1..3)");
  RPR_REQUIRE(depths && depth_tokens && depth_scores && depth_row_lo && depth_row_hi, "NULL argument");
  PrefixOuts px;
  px.n = n_depths;
  for (int k = 0; k < n_depths; ++k) {
    RPR_REQUIRE(depths[k] >= 1 && depths[k] <= L - 1 && (k == 0 || depths[k] > depths[k - 1]),
                "prefix lengths must be strictly ascending, each in [1, L-1]");
    RPR_REQUIRE(depth_tokens[k] && depth_scores[k] && depth_row_lo[k] && depth_row_hi[k], "NULL output of a prefix length");
    px.depths[k] = depths[k];
    px.tokens[k] = depth_tokens[k]; px.scores[k] = depth_scores[k]; px.lo[k] = depth_row_lo[k]; px.hi[k] = depth_row_hi[k];
  }
  return search_entry(c, m, tr, input_ids, attention_mask, Q, Lq, B, L, flags, out_tokens, out_scores, out_row_lo, out_row_hi,
                      nullptr, nullptr, stream, &px);
}

int rpr_set_lane_split(rpr_ctx* c, int32_t min_rows) {
  RPR_REQUIRE(c && min_rows >= 0, "NULL ctx or negative threshold");
  c->lane_min_rows = min_rows;
  return RPR_OK;
}
int32_t rpr_lane_split(rpr_ctx* c) {
  if (!c || c->lane_min_rows <= 0) return 0;
  (void)hipSetDevice(c->device);
  return ensure_lanes(c) ? c->lane_min_rows : 0;
}

int rpr_set_l0_table(rpr_ctx* c, int32_t mode) {
  RPR_REQUIRE(c && mode >= 0 && mode <= 2, "mode must be 0 (never), 1 (where the ping-pong GEMM would run) or 2 (always)");
  c->l0_mode = mode;
  return RPR_OK;
}
int64_t rpr_l0_table_bytes(const rpr_ctx* c, const rpr_model* m) { return c && m && m->l0_ready(c) ? (int64_t)m->l0_bytes() : 0; }

int rpr_set_gemm_mfma16(rpr_ctx* c, int32_t mode) {
  RPR_REQUIRE(c && (mode == 0 || mode == 1), "mode must be 0 (32x32x16 everywhere) or 1 (16x16x32 in the tail passes of a search)");
  c->gemm_mfma16 = mode;
  return RPR_OK;
}
int32_t rpr_gemm_mfma16(const rpr_ctx* c) { return c ? c->gemm_mfma16 : -1; }

int rpr_set_tail_extras(rpr_ctx* c, int32_t mode) {
  RPR_REQUIRE(c && mode >= -1 && mode <= 31, "mode must be -1 (automatic), 0 (off) or a budget of 1..31 extra sequences per query");
  c->tail_extras = mode;
  return RPR_OK;
}
int32_t rpr_tail_extras(const rpr_ctx* c) { return c ? c->tail_extras : -1; }

int rpr_set_forced_tail(rpr_ctx* c, int32_t mode) {
  RPR_REQUIRE(c && mode >= 0 && mode <= 2, "mode must be 0 (off), 1 (exact) or 2 (optimistic)");
  c->forced_tail = mode;
  return RPR_OK;
}
int32_t rpr_forced_tail(const rpr_ctx* c) { return c ? c->forced_tail : -1; }

int rpr_set_fork_depths(rpr_ctx* c, int32_t n, const int32_t* depths) {
  RPR_REQUIRE(c && n >= -1 && n <= MAX_FORKS && (n <= 0 || depths), "n out of range (-1 = automatic, 0..2 explicit depths)");
  c->n_fork_override = n;
  for (int i = 0; i < n; ++i) {
    RPR_REQUIRE(depths[i] >= 1 && depths[i] < 256 && (i == 0 || depths[i] > depths[i - 1]), "fork depths must be ascending and >= 1");
    c->fork_override[i] = depths[i];
  }
  return RPR_OK;
}

int rpr_fork_depths(rpr_ctx* c, rpr_model* m, rpr_trie* tr, int32_t Q, int32_t B, int32_t L, uint32_t flags, int32_t* out_depths) {
  RPR_REQUIRE(c && m && tr && out_depths, "NULL argument");
  RPR_REQUIRE(Q >= 1 && B >= 1 && L >= 1 && L <= tr->L, "Q, B or L out of range");
  const SearchPlan p = make_plan(c, m, tr, Q, 0, B, L, flags, false, false, -1);   // the plan of rpr_search (no margins) on one workspace
  for (int i = 0; i < p.n_forks; ++i) out_depths[i] = p.forks[i];
  return p.n_forks;
}

int rpr_last_fork_stats(rpr_ctx* c, int32_t* out_depths, int32_t* out_forced, int32_t* out_left) {
  RPR_REQUIRE(c && out_depths && out_forced && out_left, "NULL argument");
  RPR_HIP(hipSetDevice(c->device));
  RPR_HIP(hipDeviceSynchronize());
  const int n = (int)c->last_forks.size();
  for (int k = 0; k < n; ++k) {
    out_depths[k] = c->last_forks[(size_t)k]; out_forced[k] = 0; out_left[k] = 0;
    const Workspace* wss[3] = {&c->ws, &c->lanes[0].ws, &c->lanes[1].ws};
    for (int i = 0; i < 3; ++i) {
      if (!(c->last_ws_mask & (1 << i)) || !wss[i]->tail[k].cnt.p || !wss[i]->stage[k].cnt.p) continue;
      int32_t a = 0, b = 0;
      RPR_HIP(hipMemcpy(&a, static_cast<const char*>(wss[i]->tail[k].cnt.p) + 12, 4, hipMemcpyDeviceToHost));   // forced queries (cnt[0] counts their spare entries too)
      RPR_HIP(hipMemcpy(&b, wss[i]->stage[k].cnt.p, 4, hipMemcpyDeviceToHost));
      out_forced[k] += a; out_left[k] += b;
    }
  }
  return n;
}

int rpr_lngknp_forward(rpr_ctx* c, rpr_model* m, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz,
                       int32_t Lq, const int32_t* doc_codes, int32_t n_docs, int32_t L, const float* teacher_pos,
                       const float* teacher_neg, const int32_t* prefix_lens, int32_t n_prefix, float* out_losses,
                       float* out_position_scores, void* stream) {
  RPR_REQUIRE(c && m && input_ids && attention_mask && doc_codes, "NULL argument");
  RPR_REQUIRE(m->ctx == c, "model belongs to another ctx");
  RPR_REQUIRE(bz >= 1 && Lq >= 1 && Lq <= MAX_LQ, "bz or Lq out of range");
  RPR_REQUIRE(L >= 1 && L <= m->d.L && L <= MAX_LQ, "smtid length exceeds the model's decoder length");
  RPR_REQUIRE(n_docs >= 1 && (int64_t)bz * n_docs * L < ((int64_t)1 << 24), "n_docs out of range");
  RPR_REQUIRE(m->d.d_kv == DKV || m->d.d_kv == 128, "d_kv must be 64 (t5-base / t5-large) or 128 (t5-3b)");
  RPR_REQUIRE(n_prefix >= 0 && n_prefix <= 8, "n_prefix out of range (0..8)");
  RPR_REQUIRE(n_prefix == 0 || (n_docs == 2 && teacher_pos && teacher_neg && prefix_lens && out_losses),
              "the margin losses need n_docs == 2 (positive, negative), teacher scores, prefix lengths and out_losses");
  RPR_REQUIRE(out_losses || out_position_scores, "nothing to return");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int e = ensure_weight_planes(c, m, s);
  if (e) return e;
  e = alloc_train_workspace(c, m, bz, Lq, n_docs, L);
  if (e) return e;
  Workspace& w = c->ws;
  const size_t T = (size_t)bz * Lq, R = (size_t)bz * n_docs * L;
  RPR_HIP(hipMemcpyAsync(w.ids.p, input_ids, T * 4, hipMemcpyDeviceToDevice, s));
  RPR_HIP(hipMemcpyAsync(w.mask.p, attention_mask, T * 4, hipMemcpyDeviceToDevice, s));
  float* scores = P<float>(w.tr_misc);
  int32_t* codes = reinterpret_cast<int32_t*>(scores + R);
  RPR_HIP(hipMemcpyAsync(codes, doc_codes, R * 4, hipMemcpyDeviceToDevice, s));
  PrecGuard prec_guard(c, m);
  Launcher Ln{c, s};
  enqueue_train_forward(Ln, c, m, bz, Lq, n_docs, L, codes, scores);
  if (Ln.err) return Ln.err;
  if (n_prefix > 0)
    RPR_HIP(launch_margin_mse(scores, teacher_pos, teacher_neg, prefix_lens, n_prefix, bz, L, out_losses, nullptr, s));
  if (out_position_scores) RPR_HIP(hipMemcpyAsync(out_position_scores, scores, R * 4, hipMemcpyDeviceToDevice, s));
  return RPR_OK;
}

int rpr_encode(rpr_ctx* c, rpr_model* m, const int32_t* input_ids, const int32_t* attention_mask, int32_t Q,
               int32_t Lq, float* out, void* stream) {
  RPR_REQUIRE(c && m && input_ids && attention_mask && out, "NULL argument");
  RPR_REQUIRE(Q >= 1 && Lq >= 1 && Lq <= MAX_LQ, "Q or Lq out of range");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int e = ensure_weight_planes(c, m, s);
  if (e) return e;
  e = alloc_workspace(c, m, plain_plan(Q, Lq, 1, 1));
  if (e) return e;
  Workspace& w = c->ws;
  const size_t T = (size_t)Q * Lq;
  RPR_HIP(hipMemcpyAsync(w.ids.p, input_ids, T * 4, hipMemcpyDeviceToDevice, s));
  RPR_HIP(hipMemcpyAsync(w.mask.p, attention_mask, T * 4, hipMemcpyDeviceToDevice, s));
  PrecGuard prec_guard(c, m);
  Launcher Ln{c, s};
  enqueue_encoder(Ln, c, m, Q, Lq, false);
  if (Ln.err) return Ln.err;
  RPR_HIP(hipMemcpyAsync(out, w.enc_out.p, T * m->d.d_model * 4, hipMemcpyDeviceToDevice, s));
  return RPR_OK;
}

// Dense embedding of a text (reference T5SeqAQEncoder.query_encode / T5AQEncoder.query_encode,
// modeling/t5_generative_retriever.py:786-792, 891-897): the teacher-forced forward with one document of one position,
// ended by the normalised hidden row instead of a gold-code score.
int rpr_embed(rpr_ctx* c, rpr_model* m, const int32_t* input_ids, const int32_t* attention_mask, int32_t bz, int32_t Lq,
              float* out, void* stream) {
  RPR_REQUIRE(c && m && input_ids && attention_mask && out, "NULL argument");
  RPR_REQUIRE(m->ctx == c, "model belongs to another ctx");
  RPR_REQUIRE(bz >= 1 && bz < (1 << 24) && Lq >= 1 && Lq <= MAX_LQ, "bz or Lq out of range (Lq <= 256)");
  RPR_REQUIRE(m->d.d_kv == DKV || m->d.d_kv == 128, "d_kv must be 64 (t5-base / t5-large) or 128 (t5-3b)");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int e = ensure_weight_planes(c, m, s);
  if (e) return e;
  e = alloc_train_workspace(c, m, bz, Lq, 1, 1);
  if (e) return e;
  Workspace& w = c->ws;
  const size_t T = (size_t)bz * Lq;
  RPR_HIP(hipMemcpyAsync(w.ids.p, input_ids, T * 4, hipMemcpyDeviceToDevice, s));
  RPR_HIP(hipMemcpyAsync(w.mask.p, attention_mask, T * 4, hipMemcpyDeviceToDevice, s));
  // position 0 is fed with the start embedding (decoder_input_ids = [-1]): no code is read; the slot stays defined anyway
  int32_t* codes = reinterpret_cast<int32_t*>(P<float>(w.tr_misc) + bz);
  RPR_HIP(hipMemsetAsync(codes, 0, (size_t)bz * 4, s));
  PrecGuard prec_guard(c, m);
  Launcher Ln{c, s};
  enqueue_train_forward(Ln, c, m, bz, Lq, 1, 1, codes, P<float>(w.tr_misc), out);
  return Ln.err ? Ln.err : RPR_OK;
}

int rpr_op_linear(rpr_ctx* c, const float* A, const float* W, const float* residual, float* C, int32_t M, int32_t N,
                  int32_t K, int32_t relu, void* stream) {
  RPR_REQUIRE(c && A && W && C, "NULL argument");
  RPR_REQUIRE(M >= 1 && N >= 1 && K >= 32 && K % 32 == 0, "bad GEMM shape (K must be a multiple of 32)");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Launcher Ln{c, s};
  DevTmp At, Wt;
  PrecGuard prec_guard(c, nullptr);
  if (c->precision == RPR_PREC_F16X2) {  // test hook: split the operands on the fly
    { const int pe = ensure(c, c->ws.part, (size_t)9 << 20 << 2); if (pe) return pe; }   // split-K scratch, as a search has it
    RPR_HIP(At.alloc((size_t)M * K * 2 * sizeof(__half)));
    RPR_HIP(Wt.alloc((size_t)N * K * 2 * sizeof(__half)));
    RPR_HIP(launch_split_planes(A, At.as<__half>(), (size_t)M * K, (size_t)M * K, s, 1.0f, nullptr, 0, c->status));
    RPR_HIP(launch_split_planes(W, Wt.as<__half>(), (size_t)N * K, (size_t)N * K, s, W_PLANE_SCALE, nullptr, 0, c->status));
  }
  linear(Ln, {A, At.as<__half>(), (size_t)M * K, K, 1.0f}, {W, Wt.as<__half>(), N, K}, M, out_f32(C, N, N, residual, relu));
  if (At.p) RPR_HIP(hipStreamSynchronize(s));   // the temporaries are freed when this scope ends
  return Ln.err;
}

// Test hook: ONE split-precision launch with the epilogues a search gives it (passes.hip), on either MFMA shape of the 256x256 kernel.
int rpr_op_linear_h2(rpr_ctx* c, const float* A, const float* W, int32_t M, int32_t N, int32_t K, int32_t mode, int32_t mfma16, int32_t relu,
                     const float* resid, const uint64_t* row_ssq, float eps, const int32_t* m_dev, int32_t rm_B, int32_t split_n,
                     float* out0, float* out1, float* out2, void* out_planes, uint64_t* ssq_out, void* stream) {
  RPR_REQUIRE(c && A && W, "NULL argument");
  RPR_REQUIRE(M >= 1 && N >= 32 && N % 32 == 0 && K >= 32 && K % 32 == 0, "bad GEMM shape (N and K must be multiples of 32)");
  RPR_REQUIRE(mode >= RPR_LIN_F32 && mode <= RPR_LIN_LIVE_ROWS && (mfma16 == 0 || mfma16 == 1), "mode or mfma16 out of range");
  RPR_REQUIRE(c->precision == RPR_PREC_F16X2, "the hook launches the split-precision kernels: the ctx precision must be f16x2");
  const bool planes = mode == RPR_LIN_X_PLANES || mode == RPR_LIN_FF_PLANES;
  RPR_REQUIRE(planes ? out_planes != nullptr : out0 != nullptr, "the mode's output buffer is NULL");
  RPR_REQUIRE(mode != RPR_LIN_X_PLANES || (resid && ssq_out), "x-stream mode needs the residual and the row-sum buffer");
  RPR_REQUIRE(mode != RPR_LIN_KV_SCATTER || (out1 && out2 && rm_B >= 1 && split_n >= 64 && split_n % 64 == 0 && 3 * split_n >= N),
              "scatter mode needs out1, out2, rm_B and a split_n that is a multiple of 64 with 3 * split_n >= N");
  RPR_REQUIRE(mode != RPR_LIN_FUSED_NORM || row_ssq, "fused-norm mode needs row_ssq");
  RPR_REQUIRE(mode != RPR_LIN_LIVE_ROWS || m_dev, "live-row mode needs m_dev");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  Launcher Ln{c, s};
  Ln.mfma16 = mfma16;
  DevTmp At, Wt;
  { const int pe = ensure(c, c->ws.part, (size_t)9 << 20 << 2); if (pe) return pe; }   // split-K scratch, as a search has it
  const float a_scale = mode == RPR_LIN_FUSED_NORM ? X_PLANE_SCALE : 1.0f;            // (fused norm: A = the planes of the x stream)
  RPR_HIP(At.alloc((size_t)M * K * 2 * sizeof(__half)));
  RPR_HIP(Wt.alloc((size_t)N * K * 2 * sizeof(__half)));
  RPR_HIP(launch_split_planes(A, At.as<__half>(), (size_t)M * K, (size_t)M * K, s, a_scale, nullptr, 0, c->status));
  RPR_HIP(launch_split_planes(W, Wt.as<__half>(), (size_t)N * K, (size_t)N * K, s, W_PLANE_SCALE, nullptr, 0, c->status));
  LinIn in{A, At.as<__half>(), (size_t)M * K, K, a_scale};
  LinOut o = out_f32(out0, N, N, (mode == RPR_LIN_F32) ? resid : nullptr, relu);
  __half* oh = reinterpret_cast<__half*>(out_planes);
  if (mode == RPR_LIN_X_PLANES) {          // XStream::out: x += product, in place in the planes, with the site's row sums
    RPR_HIP(launch_split_planes(resid, oh, (size_t)M * N, (size_t)M * N, s, X_PLANE_SCALE, nullptr, 0, c->status));
    o = LinOut{};
    o.split_n = N; o.h = oh; o.ps = (size_t)M * N; o.ldh = N; o.plane_scale = X_PLANE_SCALE; o.resid_h = oh; o.ssq_out = reinterpret_cast<unsigned long long*>(ssq_out);
  } else if (mode == RPR_LIN_FF_PLANES) {   // Pass::ff_block: relu(h Wi^T) as FF-scaled planes
    o = out_f32(nullptr, N, N, nullptr, 1);
    o.h = oh; o.ps = (size_t)M * N; o.ldh = N; o.plane_scale = FF_PLANE_SCALE;
  } else if (mode == RPR_LIN_KV_SCATTER) {  // q rows | K/V-cache layout [query][head][beam][64] of the steps
    o = out_f32(out0, split_n, split_n);
    o.f[1] = out1; o.f[2] = out2;
    o.rm_B = rm_B; o.rm_slot = 64; o.rm_head = (size_t)rm_B * 64; o.rm_stride = (size_t)(split_n / 64) * rm_B * 64;
  } else if (mode == RPR_LIN_FUSED_NORM) {  // XStream::in: rows scaled by rsqrt(row_ssq / (K * SSQ_FIX) + eps)
    in.ssq = reinterpret_cast<const unsigned long long*>(row_ssq); in.inv_d_fix = 1.0f / ((float)K * SSQ_FIX); in.eps = eps;
    // (the floor test a pass runs over its row totals, passes.hip Pass::check_ssq)
    RPR_HIP(launch_ssq_floor(reinterpret_cast<unsigned long long*>(const_cast<uint64_t*>(row_ssq)), (size_t)M, in.inv_d_fix, c->status, false, s));
  }
  linear(Ln, in, {W, Wt.as<__half>(), N, K}, M, o, mode == RPR_LIN_LIVE_ROWS ? reinterpret_cast<const int*>(m_dev) : nullptr);
  RPR_HIP(hipStreamSynchronize(s));   // the temporaries are freed when this scope ends
  return Ln.err;
}

int rpr_op_linear_bf16(rpr_ctx* c, const float* A, const float* W, const float* residual, float* C, int32_t M, int32_t N, int32_t K,
                       int32_t relu, int32_t n_products, void* stream) {
  RPR_REQUIRE(c && A && W && C, "NULL argument");
  RPR_REQUIRE(M >= 1 && N >= 1 && K >= 64 && K % 64 == 0, "bad GEMM shape (K must be a multiple of 64)");
  RPR_REQUIRE(n_products >= 0 && n_products <= GemmGroupArgs::MAXP, "n_products out of range");
  RPR_REQUIRE(n_products == 0 || (!residual && !relu && (N & 3) == 0), "the grouped launch has no fused extras");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  DevTmp At, Wt, part, tab;
  RPR_HIP(At.alloc((size_t)M * K * sizeof(__half)));
  RPR_HIP(Wt.alloc((size_t)N * K * sizeof(__half)));
  RPR_HIP(launch_to_bf16(A, M, K, K, At.p, s));
  RPR_HIP(launch_to_bf16(W, N, K, K, Wt.p, s));
  if (n_products == 0) {
    const size_t part_bytes = (size_t)64 << 20;
    RPR_HIP(part.alloc(part_bytes));
    GemmH2Args g{};
    g.A = At.as<__half>(); g.lda = K; g.W = Wt.as<__half>(); g.ldw = K;
    g.resid = residual; g.ldr = N;
    g.out[0] = g.out[1] = g.out[2] = C; g.ldo[0] = g.ldo[1] = g.ldo[2] = N; g.split_n = N;
    g.M = M; g.N = N; g.K = K; g.relu = relu; g.acc_scale = 1.0f; g.bf16 = 1;
    g.part = part.as<float>(); g.part_cap = part_bytes / sizeof(float);
    Launcher Ln{c, s};                                    // (profile accounting: tools/gemm_bf16_bench.py times the launch alone)
    Ln.run(RPR_K_GEMM, 2.0 * M * (double)N * K, 2.0 * ((double)M * K + (double)N * K) + 4.0 * (double)M * N, [&] { return launch_gemm_h2(g, s); },
           &g.kernel_cls);
    if (Ln.err) return Ln.err;
  } else {
    RPR_HIP(tab.alloc(GemmGroupArgs::SCRATCH_BYTES));
    GemmGroupArgs p{};
    p.K = K; p.lda = K; p.ldw = K;
    for (int i = 0; i < n_products && M - 256 * i > 0; ++i) {
      p.A[i] = At.as<__half>(); p.W[i] = Wt.as<__half>(); p.out[i] = C + (size_t)i * M * N;
      p.M[i] = M - 256 * i; p.N[i] = N; p.ldo[i] = N;
      p.n = i + 1;
    }
    RPR_HIP(launch_gemm_h2_group(p, tab.p, s));
  }
  RPR_HIP(hipStreamSynchronize(s));   // the temporaries are freed when this scope ends
  return RPR_OK;
}

int rpr_op_rmsnorm(rpr_ctx* c, const float* x, const float* w, float* out, int32_t rows, int32_t d, float eps,
                   void* stream) {
  RPR_REQUIRE(c && x && w && out, "NULL argument");
  RPR_REQUIRE(rows >= 1 && d >= 4 && d % 4 == 0, "bad shape");
  RPR_HIP(hipSetDevice(c->device));
  RPR_HIP(launch_rmsnorm(x, w, out, rows, d, eps, reinterpret_cast<hipStream_t>(stream)));
  return RPR_OK;
}

int rpr_op_gated_gelu(rpr_ctx* c, const float* gu, int32_t M, int32_t F, const int32_t* m_dev, float* out_f32, void* out_planes,
                      void* stream) {
  RPR_REQUIRE(c && gu && (out_f32 || out_planes), "NULL argument");
  RPR_REQUIRE(M >= 1 && F >= 4 && F % 4 == 0, "bad shape");
  RPR_HIP(hipSetDevice(c->device));
  RPR_HIP(launch_gated_gelu(gu, M, F, m_dev, out_f32, reinterpret_cast<__half*>(out_planes), (size_t)M * F, c->status,
                            reinterpret_cast<hipStream_t>(stream)));
  return RPR_OK;
}

int rpr_op_gated_gelu_bwd(rpr_ctx* c, const float* gu, const float* dmid, int32_t M, int32_t F, float* dgu, void* stream) {
  RPR_REQUIRE(c && gu && dmid && dgu, "NULL argument");
  RPR_REQUIRE(M >= 1 && F >= 4 && F % 4 == 0, "bad shape");
  RPR_HIP(hipSetDevice(c->device));
  RPR_HIP(launch_gated_gelu_bwd(gu, dmid, M, F, dgu, reinterpret_cast<hipStream_t>(stream)));
  return RPR_OK;
}

// ---- attention test hooks: the descriptor -> the site's argument struct -> the site's planner (reported) and launcher ----
}  // extern "C"

namespace {

// the device bucket table of one hook call, freed on every return path
struct BucketTmp {
  int32_t* p = nullptr;
  ~BucketTmp() { if (p) (void)hipFree(p); }
};

int attn_op_common(const void* out, const void* out_planes, int64_t plane_stride, int num_buckets, int max_distance, int H, int dkv) {
  RPR_REQUIRE((out != nullptr) != (out_planes != nullptr), "exactly one of out and out_planes");
  RPR_REQUIRE(!out_planes || plane_stride > 0, "plane_stride");
  RPR_REQUIRE(num_buckets >= 2 && num_buckets <= 64 && max_distance > num_buckets, "num_buckets / max_distance out of range");
  RPR_REQUIRE(H >= 1 && (dkv == DKV || dkv == 128), "H >= 1, dkv 64 or 128");
  return RPR_OK;
}

int attn_op_plan(const AttnLaunch& p, int32_t* out_kernel, const char* site) {
  if (out_kernel) *out_kernel = p.invalid ? (int32_t)ATTN_NONE : (int32_t)p.kernel;
  if (p.invalid || p.kernel == ATTN_NONE) {
    set_error(std::string("invalid argument: the attention planner refuses this shape (") + site + ")");
    return RPR_ERR_INVALID;
  }
  return RPR_OK;
}

}  // namespace

extern "C" {

int rpr_op_enc_attn(rpr_ctx* c, const rpr_enc_attn_op* o, int32_t* out_kernel, void* stream) {
  RPR_REQUIRE(c && o && o->qkv && o->rel_bias, "NULL argument");
  if (const int e = attn_op_common(o->out, o->out_planes, o->plane_stride, o->num_buckets, o->max_distance, o->H, o->dkv)) return e;
  RPR_REQUIRE(o->Q >= 1 && o->Lq >= 1 && o->Lq <= MAX_LQ, "bad shape");
  RPR_REQUIRE(o->causal ? o->Lq <= MAX_DEC_LEN : o->mask != nullptr, "causal: Lq <= 64; bidirectional: a key mask");
  RPR_REQUIRE((o->offs != nullptr) == (o->lens != nullptr) && !(o->offs && o->causal), "offs and lens go together (bidirectional only)");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  BucketTmp bt;
  if (const int e = o->causal ? make_bucket_tables(o->num_buckets, o->max_distance, nullptr, &bt.p)
                              : make_bucket_tables(o->num_buckets, o->max_distance, &bt.p, nullptr)) return e;
  EncAttnArgs a{o->qkv, o->mask, o->rel_bias, bt.p, o->out, o->Q, o->Lq, o->H, o->num_buckets,
                reinterpret_cast<__half*>(o->out_planes), (size_t)o->plane_stride, o->offs, o->lens, c->status, o->causal ? 1 : 0, o->mfma ? 1 : 0,
                o->dkv};
  if (const int e = attn_op_plan(plan_enc_attn(enc_attn_in(a), g_attn_tuning), out_kernel, "launch_enc_attn")) return e;
  RPR_HIP(launch_enc_attn(a, s));
  RPR_HIP(hipStreamSynchronize(s));   // the bucket table is freed when this scope ends
  return RPR_OK;
}

int rpr_op_dec_self_attn(rpr_ctx* c, const rpr_dec_self_attn_op* o, int32_t* out_kernel, void* stream) {
  RPR_REQUIRE(c && o && o->q && o->kcache && o->vcache && o->anc && o->rel_bias, "NULL argument");
  if (const int e = attn_op_common(o->out, o->out_planes, o->plane_stride, o->num_buckets, o->max_distance, o->H, o->dkv)) return e;
  RPR_REQUIRE(o->Q >= 1 && o->B >= 1 && o->B <= 65536 && o->t >= 0 && o->t < MAX_DEC_LEN && o->anc_ld > o->t, "bad shape");
  RPR_REQUIRE(o->q_stride > 0 && o->h_stride > 0 && o->pos_stride > 0 && o->slot_stride >= o->dkv &&
                  ((o->q_stride | o->h_stride | o->pos_stride | o->slot_stride) & 3) == 0, "cache strides: positive multiples of 4 floats");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  BucketTmp bt;
  if (const int e = make_bucket_tables(o->num_buckets, o->max_distance, nullptr, &bt.p)) return e;
  DecSelfAttnArgs a{o->q, o->kcache, o->vcache, (size_t)o->q_stride, (size_t)o->h_stride, (size_t)o->pos_stride, (size_t)o->slot_stride,
                    o->anc, o->anc_ld, o->rel_bias, bt.p, o->out, o->Q, o->B, o->H, o->t,
                    reinterpret_cast<__half*>(o->out_planes), (size_t)o->plane_stride, c->status, o->nq_dev};
  a.dkv = o->dkv;
  if (const int e = attn_op_plan(plan_dec_self_attn(dec_self_attn_in(a)), out_kernel, "launch_dec_self_attn")) return e;
  RPR_HIP(launch_dec_self_attn(a, s));
  RPR_HIP(hipStreamSynchronize(s));
  return RPR_OK;
}

int rpr_op_cross_attn(rpr_ctx* c, const rpr_cross_attn_op* o, int32_t* out_kernel, void* stream) {
  RPR_REQUIRE(c && o && o->q && o->xk && o->xv && o->mask, "NULL argument");
  if (const int e = attn_op_common(o->out, o->out_planes, o->plane_stride, 32, 128, o->H, o->dkv)) return e;
  RPR_REQUIRE(o->site >= RPR_CROSS_SITE_BLOCK && o->site <= RPR_CROSS_SITE_TAIL, "site");
  RPR_REQUIRE(o->Q >= 1 && o->B >= 1 && o->Lq >= 1 && o->Lq <= MAX_LQ && o->xld >= o->H * o->dkv && (o->xld & 3) == 0, "bad shape");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // index of the last attended key + 1 of every query, as a search computes it (and its empty-query report)
  if (const int e = ensure(c, c->ws.last, (size_t)o->Q * sizeof(int32_t))) return e;
  RPR_HIP(launch_mask_lengths(o->mask, P<int32_t>(c->ws.last), o->Q, o->Lq, s, c->status + 1));
  DecCrossAttnArgs a{o->q, o->xk, o->xv, o->xld, o->mask, o->out, o->Q, o->B, o->H, o->Lq,
                     reinterpret_cast<__half*>(o->out_planes), (size_t)o->plane_stride, P<int32_t>(c->ws.last), o->offs, 0, c->status, o->nq_dev};
  a.dkv = o->dkv;
  const CrossAttnIn in = cross_attn_in(a);
  const AttnLaunch p = o->site == RPR_CROSS_SITE_BLOCK ? plan_cross_block(in)
                       : o->site == RPR_CROSS_SITE_STEP ? plan_step_cross_attn(in, g_attn_tuning) : plan_tail_cross_attn(in, g_attn_tuning);
  if (const int e = attn_op_plan(p, out_kernel, o->site == RPR_CROSS_SITE_BLOCK ? "launch_dec_cross_attn"
                                                : o->site == RPR_CROSS_SITE_STEP ? "launch_step_cross_attn" : "launch_tail_cross_attn")) return e;
  const hipError_t launched = o->site == RPR_CROSS_SITE_BLOCK ? launch_dec_cross_attn(a, s)
                              : o->site == RPR_CROSS_SITE_STEP ? launch_step_cross_attn(a, s) : launch_tail_cross_attn(a, s);
  RPR_HIP(launched);
  RPR_HIP(hipStreamSynchronize(s));
  return RPR_OK;
}

int rpr_op_tail_self_attn(rpr_ctx* c, const rpr_tail_self_attn_op* o, int32_t* out_kernel, void* stream) {
  RPR_REQUIRE(c && o && o->qkv && o->kcache && o->vcache && o->anc && o->flist && o->nseq_dev && o->rel_bias, "NULL argument");
  if (const int e = attn_op_common(o->out, o->out_planes, o->plane_stride, o->num_buckets, o->max_distance, o->H, o->dkv)) return e;
  RPR_REQUIRE(o->nseq_cap >= 1 && o->B >= 1 && o->nseq_cap % o->B == 0 && o->L >= 1 && o->anc_ld >= o->L, "bad shape");   // T and L: the planner
  RPR_REQUIRE(o->q_stride > 0 && o->h_stride > 0 && o->pos_stride > 0 && o->slot_stride >= o->dkv &&
                  ((o->q_stride | o->h_stride | o->pos_stride | o->slot_stride) & 3) == 0, "cache strides: positive multiples of 4 floats");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  BucketTmp bt;
  if (const int e = make_bucket_tables(o->num_buckets, o->max_distance, nullptr, &bt.p)) return e;
  TailSelfAttnArgs a{o->qkv, o->kcache, o->vcache, (size_t)o->q_stride, (size_t)o->h_stride, (size_t)o->pos_stride, (size_t)o->slot_stride,
                     o->anc, o->anc_ld, o->flist, o->nseq_dev, o->rel_bias, bt.p, o->out, reinterpret_cast<__half*>(o->out_planes),
                     (size_t)o->plane_stride, c->status, o->nseq_cap, o->B, o->H, o->T, o->L};
  a.dkv = o->dkv;
  a.kvq = o->kvq;
  if (const int e = attn_op_plan(plan_tail_self_attn(tail_self_attn_in(a), g_attn_tuning), out_kernel, "launch_tail_self_attn")) return e;
  RPR_HIP(launch_tail_self_attn(a, s));
  RPR_HIP(hipStreamSynchronize(s));
  return RPR_OK;
}

}  // extern "C"

namespace {

// the dropout block of a training attention hook -> the DropAttn the step hands its launchers (dropout.h); *on = rate > 0
int attn_op_drop(const rpr_attn_drop& d, DropAttn* da, bool* on) {
  RPR_REQUIRE(d.rate >= 0.f && d.rate < 1.f, "dropout rate in [0, 1)");
  *on = d.rate > 0.f;
  RPR_REQUIRE(!*on || (d.site >= 0 && d.site < 65536 && d.L >= 0 && d.L <= 65536), "dropout site / L out of range");
  *da = drop_attn(drop_key(d.rate, d.seed, d.step), d.site, d.L);
  return RPR_OK;
}

int train_self_attn_op_common(const rpr_ctx* c, const rpr_train_self_attn_op* o) {
  RPR_REQUIRE(c && o && o->qkv && o->rel_bias, "NULL argument");
  RPR_REQUIRE(o->num_buckets >= 2 && o->num_buckets <= 64 && o->max_distance > o->num_buckets, "num_buckets / max_distance out of range");
  RPR_REQUIRE(o->H >= 1 && (o->dkv == DKV || o->dkv == 128), "H >= 1, dkv 64 or 128");
  RPR_REQUIRE(o->S >= 1 && o->Ls >= 1 && o->Ls <= MAX_LQ, "bad shape");
  RPR_REQUIRE(o->causal ? o->mask == nullptr : o->mask != nullptr, "causal: no mask; bidirectional: a key mask");
  RPR_REQUIRE(!o->causal || o->Ls <= MAX_DEC_LEN, "causal: Ls <= 64 (the unidirectional bucket table)");
  return RPR_OK;
}

int train_cross_attn_op_common(const rpr_ctx* c, const rpr_train_cross_attn_op* o) {
  RPR_REQUIRE(c && o && o->q && o->xk && o->xv && o->mask, "NULL argument");
  RPR_REQUIRE(o->H >= 1 && (o->dkv == DKV || o->dkv == 128), "H >= 1, dkv 64 or 128");
  RPR_REQUIRE(o->bz >= 1 && o->n >= 1 && o->Lq >= 1 && o->Lq <= MAX_LQ && o->xld >= o->H * o->dkv && (o->xld & 3) == 0, "bad shape");
  return RPR_OK;
}

}  // namespace

extern "C" {

int rpr_op_train_self_attn_bwd(rpr_ctx* c, const rpr_train_self_attn_op* o, int32_t* out_kernel, void* stream) {
  if (const int e = train_self_attn_op_common(c, o)) return e;
  RPR_REQUIRE(o->dO && o->dqkv && o->dbias, "NULL argument");
  DropAttn da;
  bool drop;
  if (const int e = attn_op_drop(o->drop, &da, &drop)) return e;
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const TrainSelfAttnIn in{o->S, o->Ls, o->H, o->num_buckets, o->dkv, o->causal != 0, o->mask != nullptr, drop, drop ? da.L : 0};
  if (const int e = attn_op_plan(plan_train_self_attn_bwd(in), out_kernel, "launch_self_attn_bwd")) return e;
  BucketTmp bt;
  if (const int e = o->causal ? make_bucket_tables(o->num_buckets, o->max_distance, nullptr, &bt.p)
                              : make_bucket_tables(o->num_buckets, o->max_distance, &bt.p, nullptr)) return e;
  // the per-(sequence, head) parts of the bias gradient, as the step keeps them
  if (const int e = ensure(c, c->ws.tr_misc, (size_t)o->S * o->H * o->num_buckets * sizeof(float))) return e;
  RPR_HIP(launch_self_attn_bwd(o->qkv, o->dO, o->mask, o->rel_bias, bt.p, o->dqkv, P<float>(c->ws.tr_misc), o->dbias, o->S, o->Ls, o->H,
                               o->num_buckets, o->causal ? 1 : 0, s, drop ? &da : nullptr, o->dkv));
  RPR_HIP(hipStreamSynchronize(s));   // the bucket table is freed when this scope ends
  return RPR_OK;
}

int rpr_op_train_self_attn_drop_fwd(rpr_ctx* c, const rpr_train_self_attn_op* o, int32_t* out_kernel, void* stream) {
  if (const int e = train_self_attn_op_common(c, o)) return e;
  RPR_REQUIRE(o->out, "NULL argument");
  DropAttn da;
  bool drop;
  if (const int e = attn_op_drop(o->drop, &da, &drop)) return e;
  RPR_REQUIRE(drop, "the forward with dropped-out probabilities needs a rate > 0");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const TrainSelfAttnIn in{o->S, o->Ls, o->H, o->num_buckets, o->dkv, o->causal != 0, o->mask != nullptr, true, da.L};
  if (const int e = attn_op_plan(plan_train_self_attn_drop_fwd(in), out_kernel, "launch_self_attn_drop_fwd")) return e;
  BucketTmp bt;
  if (const int e = o->causal ? make_bucket_tables(o->num_buckets, o->max_distance, nullptr, &bt.p)
                              : make_bucket_tables(o->num_buckets, o->max_distance, &bt.p, nullptr)) return e;
  RPR_HIP(launch_self_attn_drop_fwd(o->qkv, o->mask, o->rel_bias, bt.p, o->out, o->S, o->Ls, o->H, o->num_buckets, o->causal ? 1 : 0, da, s,
                                    o->dkv));
  RPR_HIP(hipStreamSynchronize(s));
  return RPR_OK;
}

int rpr_op_train_cross_attn_bwd(rpr_ctx* c, const rpr_train_cross_attn_op* o, int32_t* out_kernel, void* stream) {
  if (const int e = train_cross_attn_op_common(c, o)) return e;
  RPR_REQUIRE(o->dO && o->dq && o->dxk && o->dxv, "NULL argument");
  DropAttn da;
  bool drop;
  if (const int e = attn_op_drop(o->drop, &da, &drop)) return e;
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const TrainCrossAttnIn in{o->bz, o->n, o->Lq, o->H, o->dkv, true, drop, drop ? da.L : 0};
  if (const int e = attn_op_plan(plan_train_cross_attn_bwd(in), out_kernel, "launch_cross_attn_bwd")) return e;
  RPR_HIP(launch_cross_attn_bwd(o->q, o->xk, o->xv, o->xld, o->mask, o->dO, o->dq, o->dxk, o->dxv, o->bz, o->n, o->Lq, o->H, s,
                                drop ? &da : nullptr, o->dkv));
  RPR_HIP(hipStreamSynchronize(s));
  return RPR_OK;
}

int rpr_op_train_cross_attn_drop_fwd(rpr_ctx* c, const rpr_train_cross_attn_op* o, int32_t* out_kernel, void* stream) {
  if (const int e = train_cross_attn_op_common(c, o)) return e;
  RPR_REQUIRE(o->out, "NULL argument");
  DropAttn da;
  bool drop;
  if (const int e = attn_op_drop(o->drop, &da, &drop)) return e;
  RPR_REQUIRE(drop, "the forward with dropped-out probabilities needs a rate > 0");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const TrainCrossAttnIn in{o->bz, o->n, o->Lq, o->H, o->dkv, true, true, da.L};
  if (const int e = attn_op_plan(plan_train_cross_attn_drop_fwd(in), out_kernel, "launch_cross_attn_drop_fwd")) return e;
  RPR_HIP(launch_cross_attn_drop_fwd(o->q, o->xk, o->xv, o->xld, o->mask, o->out, o->bz, o->n, o->Lq, o->H, da, s, o->dkv));
  RPR_HIP(hipStreamSynchronize(s));
  return RPR_OK;
}

// ---- the row-wise kernels of the training step: the descriptor -> the launcher the step calls (include/ripor_hip.h) ----
int rpr_op_train_rows(rpr_ctx* c, const rpr_train_rows_op* o, void* stream) {
  RPR_REQUIRE(c && o, "NULL argument");
  RPR_REQUIRE(o->op >= 0 && o->op < RPR_TR_COUNT, "unknown op");
  const int32_t* n = o->dims;
  const float eps = o->f[0], post = o->f[1];
  auto F = [&](int i) { return reinterpret_cast<const float*>(o->src[i]); };
  auto I = [&](int i) { return reinterpret_cast<const int32_t*>(o->src[i]); };
  auto OF = [&](int i) { return reinterpret_cast<float*>(o->dst[i]); };
  auto OI = [&](int i) { return reinterpret_cast<int32_t*>(o->dst[i]); };
  auto OH = [&](int i) { return reinterpret_cast<__half*>(o->dst[i]); };
  auto OU = [&](int i) { return reinterpret_cast<unsigned long long*>(o->dst[i]); };
  auto have = [&](int ns, int nd) {
    for (int i = 0; i < ns; ++i) if (!o->src[i]) return false;
    for (int i = 0; i < nd; ++i) if (!o->dst[i]) return false;
    return true;
  };
  auto pos = [&](int k) { for (int i = 0; i < k; ++i) if (n[i] < 1) return false; return true; };
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  DevTmp t0, t1;
  switch (o->op) {
    case RPR_TR_RMSNORM_BWD:
      RPR_REQUIRE(have(3, 2), "NULL argument");
      RPR_REQUIRE(pos(2) && n[1] % 4 == 0 && n[1] <= 4096, "bad shape (rows >= 1, d a multiple of 4, d <= 4096: four rows of d floats in 64 KB of LDS)");
      RPR_HIP(launch_rmsnorm_bwd(F(0), F(1), F(2), F(3), OF(0), OF(1), OF(2), n[0], n[1], eps, post, n[2] ? 1 : 0, s));
      break;
    case RPR_TR_COLSUM_MULTI: {
      RPR_REQUIRE(n[0] >= 1 && n[1] >= 1 && n[1] <= ColsumSites::MAXS, "bad shape (d >= 1, 1 .. 4 sites)");
      ColsumSites p{};
      p.n = n[1];
      for (int i = 0; i < p.n; ++i) {
        RPR_REQUIRE(o->src[i] && o->dst[i] && n[2 + i] >= 1, "NULL argument / nparts < 1");
        p.part[i] = F(i); p.out[i] = OF(i); p.nparts[i] = n[2 + i];
      }
      RPR_HIP(launch_colsum_multi(p, n[0], s));
      break;
    }
    case RPR_TR_GOLD_SCORES: {
      const bool hid = o->dst[1] != nullptr;
      RPR_REQUIRE(o->src[1] && o->src[2] && (o->src[0] != nullptr) != (o->src[4] != nullptr), "ln, out_embeds and exactly one of x, x_planes");
      RPR_REQUIRE((o->dst[0] != nullptr) != hid && (hid || o->src[3]), "exactly one of scores (with codes) and hidden");
      RPR_REQUIRE(pos(4) && n[2] % 4 == 0 && (!o->src[4] || n[4] >= n[0] * n[1] * n[2]), "bad shape");
      // hidden mode forms no score, but the kernel still loads row (i, 0) of out_embeds (rpr_embed passes the model's codebook)
      RPR_HIP(launch_gold_scores(F(0), F(1), F(2), I(3), OF(0), n[0], n[1], n[2], n[3], eps, post, s,
                                 reinterpret_cast<const __half*>(o->src[4]), (size_t)n[4], OF(1)));
      break;
    }
    case RPR_TR_GOLD_SCORE_BWD:
      RPR_REQUIRE(have(5, 2), "NULL argument");
      RPR_REQUIRE(pos(2) && n[1] % 4 == 0, "bad shape");
      RPR_HIP(launch_gold_score_bwd(F(0), F(1), F(2), I(3), F(4), OF(0), OF(1), n[0], n[1], eps, post, s));
      break;
    case RPR_TR_GOLD_ROWDOT:
      RPR_REQUIRE(have(3, 0) && (o->src[3] ? (o->dst[1] && o->dst[2]) : o->dst[0] != nullptr), "NULL argument");
      RPR_REQUIRE(pos(2) && n[1] % 4 == 0, "bad shape");
      RPR_HIP(launch_gold_rowdot(F(0), F(1), I(2), OF(0), F(3), OF(1), OF(2), n[0], n[1], s));
      break;
    case RPR_TR_MARGIN_MSE:
      RPR_REQUIRE(have(4, 1), "NULL argument");
      RPR_REQUIRE(pos(3), "bad shape");
      RPR_HIP(launch_margin_mse(F(0), F(1), F(2), I(3), n[0], n[1], n[2], OF(0), OF(1), s));
      break;
    case RPR_TR_MARGIN_MSE_BWD:
      RPR_REQUIRE(have(4, 1), "NULL argument");
      RPR_REQUIRE(pos(3), "bad shape");
      RPR_HIP(launch_margin_mse_bwd(F(0), F(1), F(2), I(3), n[0], n[1], n[2], OF(0), s));
      break;
    case RPR_TR_DENSE_MSE_FWD:
      RPR_REQUIRE(have(3, 4), "NULL argument");
      RPR_REQUIRE(pos(2), "bad shape");
      RPR_HIP(launch_dense_mse_head_fwd(F(0), F(1), F(2), OF(0), OF(1), OF(2), OF(3), n[0], n[1], s));
      break;
    case RPR_TR_DENSE_MSE_BWD:
      RPR_REQUIRE(have(2, 1), "NULL argument");
      RPR_REQUIRE(pos(2), "bad shape");
      RPR_HIP(launch_dense_mse_head_bwd(F(0), F(1), OF(0), n[0], n[1], s));
      break;
    case RPR_TR_RELU_BWD:
      RPR_REQUIRE(have(1, 1), "NULL argument");
      RPR_REQUIRE(n[0] >= 4 && n[0] % 4 == 0, "bad shape (n a multiple of 4)");
      RPR_HIP(launch_relu_bwd(OF(0), F(0), (size_t)n[0], s));
      break;
    case RPR_TR_DEC_EMBED: {
      RPR_REQUIRE(have(3, 0) && (o->dst[0] != nullptr) != (o->dst[1] != nullptr), "NULL argument / exactly one of out and planes");
      RPR_REQUIRE(pos(4) && n[2] % 4 == 0 && (!o->dst[1] || n[4] >= n[0] * n[1] * n[2]), "bad shape");
      XOut xo{};
      xo.x_h = OH(1); xo.x_ps = (size_t)n[4]; xo.ssq = OU(2); xo.sat = c->status;
      RPR_HIP(launch_train_dec_embed(F(0), F(1), I(2), OF(0), n[0], n[1], n[2], n[3], s, xo));
      break;
    }
    case RPR_TR_TRAIN_INDICES:
      RPR_REQUIRE(have(1, 2), "NULL argument");
      RPR_REQUIRE(pos(3), "bad shape");
      RPR_HIP(launch_train_indices(I(0), OI(0), OI(1), n[0], n[1], n[2], s));
      break;
    case RPR_TR_SCATTER_FIX:
      RPR_REQUIRE(have(2, 1), "NULL argument");
      RPR_REQUIRE(pos(2), "bad shape");
      RPR_HIP(launch_scatter_rows_fix(F(0), I(1), OU(0), n[0], n[1], s));
      break;
    case RPR_TR_FIX_FLUSH:
      RPR_REQUIRE(have(0, 2), "NULL argument");
      RPR_REQUIRE(pos(1), "bad shape");
      RPR_HIP(launch_fix_flush(OU(0), OF(1), (size_t)n[0], s));
      break;
    case RPR_TR_SUM_SELECTED:
      RPR_REQUIRE(have(2, 1), "NULL argument");
      RPR_REQUIRE(pos(2), "bad shape");
      RPR_HIP(launch_sum_selected_rows(F(0), I(1), OF(0), n[0], n[1], s));
      break;
    case RPR_TR_S2S_HEAD_FWD:
      RPR_REQUIRE(have(3, 2) && o->dst[3], "NULL argument");
      RPR_REQUIRE(pos(4) && n[2] % 32 == 0 && s2s_head_smem_ok(n[3]), "bad shape (d % 32 == 0, V % 64 == 0, V <= 1024)");
      RPR_HIP(launch_s2s_head_fwd(F(0), F(1), I(2), OF(0), OF(1), OF(2), OF(3), n[0], n[1], n[2], n[3], s));
      break;
    case RPR_TR_S2S_HEAD_BWD:
      RPR_REQUIRE(have(3, 2), "NULL argument");
      RPR_REQUIRE(pos(4) && n[2] % 32 == 0 && s2s_head_smem_ok(n[3]), "bad shape (d % 32 == 0, V % 64 == 0, V <= 1024)");
      RPR_HIP(launch_s2s_head_bwd(F(0), F(1), F(2), OF(0), OF(1), n[0], n[1], n[2], n[3], s));
      break;
    case RPR_TR_ABSMAX2:
      RPR_REQUIRE(have(1, 1), "NULL argument");
      RPR_REQUIRE(n[0] >= 1 && (!o->src[1] || n[1] >= 1), "bad shape");
      RPR_HIP(launch_absmax2(F(0), (size_t)n[0], F(1), o->src[1] ? (size_t)n[1] : 0, OF(0), s));
      break;
    case RPR_TR_SPLIT_DYN:
      RPR_REQUIRE(have(2, 1), "NULL argument");
      RPR_REQUIRE(pos(3) && n[1] % 4 == 0 && n[2] % 4 == 0 && n[2] >= n[1], "bad shape");
      RPR_HIP(launch_split_dyn(F(0), n[0], n[1], n[2], OH(0), F(1), s));
      break;
    case RPR_TR_SPLIT_DYN_T:
      RPR_REQUIRE(have(2, 1), "NULL argument");
      RPR_REQUIRE(pos(4) && n[1] % 4 == 0 && n[2] % 4 == 0 && n[2] >= n[1] && n[3] % 2 == 0 && n[3] >= n[0], "bad shape");
      RPR_HIP(launch_split_dyn_T(F(0), n[0], n[1], n[2], n[3], OH(0), OH(1), F(1), s));
      break;
    case RPR_TR_TO_BF16:
      RPR_REQUIRE(have(1, 1), "NULL argument");
      RPR_REQUIRE(pos(3) && n[1] % 4 == 0 && n[2] % 4 == 0 && n[2] >= n[1], "bad shape");
      RPR_HIP(launch_to_bf16(F(0), n[0], n[1], n[2], o->dst[0], s));
      break;
    case RPR_TR_TO_BF16_T:
      RPR_REQUIRE(have(1, 1), "NULL argument");
      RPR_REQUIRE(pos(4) && n[1] % 4 == 0 && n[2] % 4 == 0 && n[2] >= n[1] && n[3] % 2 == 0 && n[3] >= n[0] &&
                      (n[4] == 0 || (n[4] % 2 == 0 && n[4] >= n[3])), "bad shape");
      RPR_HIP(launch_to_bf16_T(F(0), n[0], n[1], n[2], n[3], o->dst[0], o->dst[1], s, F(1), n[4]));
      break;
    case RPR_TR_RMSNORM_BF16_T:
      RPR_REQUIRE(have(2, 2), "NULL argument");
      RPR_REQUIRE(pos(4) && n[1] <= 1024 && n[1] % 8 == 0 && n[2] % 32 == 0 && n[2] >= n[0] && n[3] % 8 == 0 && n[3] >= n[2],
                  "bad shape (d <= 1024, d % 8 == 0, Rpad % 32 == 0, Rpad >= rows, ldt % 8 == 0, ldt >= Rpad)");
      RPR_HIP(launch_rmsnorm_bf16_T(F(0), F(1), n[0], n[1], eps, post, o->dst[0], o->dst[1], n[2], n[3], s));
      break;
    case RPR_TR_WEIGHTS_BF16: {
      RPR_REQUIRE(o->dst[0] && o->dst[1] && n[0] >= 1 && n[0] <= 5, "NULL argument / 1 .. 5 segments");
      WSeg segs[5];
      int pref[5], tiles = 0;
      unsigned long long off = 0;
      for (int i = 0; i < n[0]; ++i) {    // the table the step builds in bf16_weights (train_api.hip)
        const int R = n[1 + 2 * i], Cc = n[2 + 2 * i];
        RPR_REQUIRE(o->src[i] && R >= 2 && Cc >= 4 && !(R & 1) && !(Cc & 3), "segment: R even, C a multiple of 4");
        segs[i] = WSeg{F(i), R, Cc, off};
        pref[i] = tiles;
        tiles += ((R + 63) / 64) * ((Cc + 63) / 64);
        off += (unsigned long long)R * Cc;
      }
      RPR_HIP(t0.alloc(sizeof(segs)));
      RPR_HIP(t1.alloc(sizeof(pref)));
      RPR_HIP(hipMemcpyAsync(t0.p, segs, n[0] * sizeof(WSeg), hipMemcpyHostToDevice, s));
      RPR_HIP(hipMemcpyAsync(t1.p, pref, n[0] * sizeof(int), hipMemcpyHostToDevice, s));
      RPR_HIP(hipStreamSynchronize(s));
      RPR_HIP(launch_weights_bf16(t0.as<WSeg>(), t1.as<int>(), n[0], tiles, o->dst[0], o->dst[1], s));
      break;
    }
    case RPR_TR_TRANSPOSE_PAD:
      RPR_REQUIRE(have(1, 1), "NULL argument");
      RPR_REQUIRE(pos(4) && n[2] >= n[1] && n[3] >= n[0], "bad shape");
      RPR_HIP(launch_transpose_pad(F(0), OF(0), n[0], n[1], n[2], n[3], s));
      break;
    default: RPR_REQUIRE(false, "unknown op");
  }
  RPR_HIP(hipStreamSynchronize(s));   // the temporaries are freed when this scope ends
  return RPR_OK;
}

const char* rpr_attn_kernel_name(int kernel) { return kernel >= 0 && kernel < ATTN_KERNEL_COUNT ? attn_kernel_name(kernel) : nullptr; }
int rpr_attn_kernel_count(void) { return ATTN_KERNEL_COUNT; }

int rpr_get_status(rpr_ctx* c, void* stream, uint32_t* out_flags, int clear) {
  RPR_REQUIRE(c && out_flags, "NULL argument");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  RPR_HIP(hipMemcpyAsync(c->status_host, c->status, 16, hipMemcpyDeviceToHost, s));
  if (clear) RPR_HIP(hipMemsetAsync(c->status, 0, 16, s));
  RPR_HIP(hipStreamSynchronize(s));
  *out_flags = (c->status_host[0] ? RPR_STATUS_SATURATED : 0u) | (c->status_host[1] ? RPR_STATUS_EMPTY_QUERY : 0u) |
               (c->status_host[2] ? RPR_STATUS_TAIL_LEFTOVER : 0u) | (c->status_host[STATUS_WORD_SMALL] ? RPR_STATUS_SMALL_STREAM : 0u);
  return RPR_OK;
}

int rpr_status_words_async(rpr_ctx* c, void* stream, uint32_t* host_words, int clear) {
  RPR_REQUIRE(c, "NULL ctx");
  RPR_HIP(hipSetDevice(c->device));
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (host_words) RPR_HIP(hipMemcpyAsync(host_words, c->status, 16, hipMemcpyDeviceToHost, s));
  if (clear) RPR_HIP(hipMemsetAsync(c->status, 0, 16, s));
  return RPR_OK;
}

int rpr_model_f32_only(const rpr_model* m) { return m ? (m->f32_only ? 1 : 0) : -1; }   // as of the last plane split

int rpr_profile_enable(rpr_ctx* c, int enable) {
  RPR_REQUIRE(c, "NULL ctx");
  if (!enable && c->profiling) { int e = flush_profile(c); if (e) return e; }
  c->profiling = enable != 0;
  return RPR_OK;
}

int rpr_profile_reset(rpr_ctx* c) {
  RPR_REQUIRE(c, "NULL ctx");
  int e = flush_profile(c);
  if (e) return e;
  std::memset(c->done, 0, sizeof(c->done));
  return RPR_OK;
}

int rpr_profile_get(rpr_ctx* c, int cls, rpr_kernel_stats* out) {
  RPR_REQUIRE(c && out, "NULL argument");
  RPR_REQUIRE(cls >= 0 && cls < RPR_K_COUNT, "bad kernel class");
  int e = flush_profile(c);
  if (e) return e;
  *out = c->done[cls];
  return RPR_OK;
}

}  // extern "C"
