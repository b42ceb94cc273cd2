// Prints the training step's layout (ripor_amd/csrc/train_layout.h) for tests/test_train_layout.py as one JSON object.
//   key=value ...   model: vocab buckets H dkv dm dff ne nd Lm V own_out (codebooks of their own: 1)   batch: bz Lq L docs
// "dims": the TrainDims; "enc" / "dec": a stack's table, strides and the offsets of every layer; "params": the flat order;
// "index_ok": ParamOrder::index finds every slot at its own position; "weights": the GEMM weights of every sub-block as the
// loader and the forward passes get them; "fields": the ABI's field of every layer slot (null_field= null_elem=: see print_fields).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../ripor_amd/csrc/train_layout.h"

using namespace rpr;

static void print_stack(const char* name, const StackLayout& st, const ParamOrder& po) {
  printf("\"%s\": {\"rows\": %d, \"ld\": %d, \"layers\": %d, \"act_stride\": %zu, \"xt_base\": %zu, \"xt_stride\": %zu, \"dyT_elems\": %zu, \"sub\": [",
         name, st.rows, st.ld, st.layers, st.act_stride, st.xt_base, st.xt_stride, st.dyT_elems);
  for (int j = 0; j < st.nsub; ++j)
    printf("%s{\"kind\": %d, \"n_in\": %d, \"k_out\": %d}", j ? ", " : "", (int)st.sub[j].kind, st.sub[j].n_in, st.sub[j].k_out);
  printf("], \"layer\": [");
  for (int i = 0; i < st.layers; ++i) {   // per layer: per sub-block [x, in, mid, xt_in, xt_out], then the bucket [offset, numel]
    printf("%s{\"at\": [", i ? ", " : "");
    for (int j = 0; j < st.nsub; ++j) {
      const SubSlots& a = st.at[j];
      printf("%s[%zu, %zu, %zu, %zu, %zu]", j ? ", " : "", st.act(i, a.x), st.act(i, a.in), st.act(i, a.mid), st.xt(i, a.xt_in), st.xt(i, a.xt_out));
    }
    size_t off, numel;
    po.bucket(st, i, &off, &numel);
    printf("], \"first_param\": %d, \"bucket\": [%zu, %zu]}", (int)(po.sub(st, i, 0) - po.slots.data()), off, numel);
  }
  printf("], \"x_end\": %zu}", st.act(st.layers, st.at[0].x));
}

// per layer and sub-block: the slot of ln, then W_in and W_out as [slot, numel, N, K, slot of the folded norm weight or -1]
static void print_weights(const char* name, bool dec, const ParamOrder& po) {
  const StackLayout& st = po.stack[dec];
  printf("\"%s\": [", name);
  for (int i = 0; i < st.layers; ++i) {
    printf("%s[", i ? ", " : "");
    for (int j = 0; j < st.nsub; ++j) {
      printf("%s{\"ln\": %d", j ? ", " : "", (int)(po.sub(st, i, j) - po.slots.data()));
      for (int role = P_WIN; role <= P_WOUT; ++role) {
        const WeightRef r = po.weight(dec, i, j, role);
        printf(", \"%s\": [%d, %zu, %d, %d, %d]", role == P_WIN ? "w_in" : "w_out", r.slot, po.slots[(size_t)r.slot].numel, r.N, r.K, r.fold);
      }
      printf("}");
    }
    printf("]");
  }
  printf("]");
}

// ParamOrder::fill against a desc of two encoder and three decoder layers whose 15 per-layer arrays hold the addresses
// cell[field][layer], the fields assigned BY NAME in the order of the ABI's documentation. Prints [kind, layer, field,
// element] of every layer slot and what fill returned. null_field >= 0: that array lacks element null_elem (-1: the array).
static void print_fields(int null_field, int null_elem) {
  static float cell[15][3];
  const float* arr[15][3];
  for (int f = 0; f < 15; ++f) for (int e = 0; e < 3; ++e) arr[f][e] = &cell[f][e];
  if (null_field >= 0 && null_elem >= 0) arr[null_field][null_elem] = nullptr;
  static float global;
  rpr_model_desc d;
  memset(&d, 0, sizeof d);
  d.vocab_size = 8; d.d_model = 32; d.d_kv = 64; d.d_ff = 32; d.num_heads = 1; d.num_layers = 2; d.num_decoder_layers = 3;
  d.rel_buckets = 2; d.L = 1; d.V = 2;
  d.shared = d.enc_rel_bias = d.dec_rel_bias = d.enc_final_ln = d.dec_final_ln = d.start_embed = d.in_embeds = d.out_embeds = d.dec_xkv = &global;
  d.enc_ln0 = arr[0]; d.enc_qkv = arr[1]; d.enc_o = arr[2]; d.enc_ln1 = arr[3]; d.enc_wi = arr[4]; d.enc_wo = arr[5];
  d.dec_ln0 = arr[6]; d.dec_qkv = arr[7]; d.dec_o = arr[8]; d.dec_ln1 = arr[9]; d.dec_xq = arr[10]; d.dec_xo = arr[11];
  d.dec_ln2 = arr[12]; d.dec_wi = arr[13]; d.dec_wo = arr[14];
  if (null_field >= 0 && null_elem < 0) d.*layer_field(K_ENC_LAYER + null_field) = nullptr;
  ParamOrder po(d);
  const bool ok = po.fill(d);
  printf("\"fields\": {\"fill_ok\": %d, \"globals_ok\": %d, \"slots\": [", (int)ok, (int)(po.at(K_XKV).ptr == &global && po.at(K_SHARED).ptr == &global));
  bool first = true;
  for (const ParamSlot& p : po.slots) {
    if (p.kind < K_ENC_LAYER || !p.ptr) continue;
    const ptrdiff_t at = p.ptr - &cell[0][0];
    printf("%s[%d, %d, %d, %d]", first ? "" : ", ", p.kind, p.layer, (int)(at / 3), (int)(at % 3));
    first = false;
  }
  printf("]}");
}

int main(int argc, char** argv) {
  rpr_model_desc d;
  memset(&d, 0, sizeof d);
  int bz = 1, Lq = 1, L = 1, docs = 2, own_out = 1, null_field = -1, null_elem = -1;
  for (int i = 1; i < argc; ++i) {
    const char* eq = strchr(argv[i], '=');
    if (!eq) { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
    const std::string k(argv[i], eq - argv[i]);
    const int v = atoi(eq + 1);
    if (k == "vocab") d.vocab_size = v; else if (k == "buckets") d.rel_buckets = v; else if (k == "H") d.num_heads = v;
    else if (k == "dkv") d.d_kv = v; else if (k == "dm") d.d_model = v; else if (k == "dff") d.d_ff = v;
    else if (k == "ne") d.num_layers = v; else if (k == "nd") d.num_decoder_layers = v; else if (k == "Lm") d.L = v;
    else if (k == "V") d.V = v; else if (k == "own_out") own_out = v; else if (k == "bz") bz = v; else if (k == "Lq") Lq = v;
    else if (k == "L") L = v; else if (k == "docs") docs = v; else if (k == "null_field") null_field = v; else if (k == "null_elem") null_elem = v;
    else { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
  }
  static float in_emb, out_emb;   // only their identity is read: shared codebooks are one tensor
  d.in_embeds = &in_emb;
  d.out_embeds = own_out ? &out_emb : &in_emb;
  d.layer_norm_eps = 1e-6f;
  const TrainDims D = train_dims(d, bz, Lq, L, docs);
  const TrainLayout Y(D);
  const ParamOrder po(d);
  printf("{\"dims\": {\"S\": %d, \"R\": %d, \"T\": %d, \"inner\": %d, \"xld\": %d}, ", D.S, D.R, D.T, D.inner, D.xld);
  print_stack("enc", Y.enc, po);
  printf(", ");
  print_stack("dec", Y.dec, po);
  printf(", \"weights\": {");
  print_weights("enc", false, po);
  printf(", ");
  print_weights("dec", true, po);
  printf("}, ");
  print_fields(null_field, null_elem);
  printf(", \"xt_xkv\": %zu, \"xt_total\": %zu, \"dyT_xkv\": %zu, \"dyT_max\": %zu, \"params\": [", Y.xt_xkv, Y.xt_total, Y.dyT_xkv, Y.dyT_max());
  bool index_ok = true;
  for (size_t i = 0; i < po.slots.size(); ++i) {
    const ParamSlot& p = po.slots[i];
    index_ok = index_ok && po.index(p.kind, p.layer) == (int)i;
    printf("%s[%d, %d, %zu, %zu]", i ? ", " : "", p.kind, p.layer, p.numel, p.offset);
  }
  printf("], \"params_total\": %zu, \"index_ok\": %d, \"first_bucket\": [0, %zu]}\n", po.total, (int)index_ok, po.at(K_ENC_LAYER, 0).offset);
  return 0;
}
