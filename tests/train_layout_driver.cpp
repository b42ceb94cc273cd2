// Prints the training step's layout (ripor_amd/csrc/train_layout.h) for tests/test_train_layout.py as one JSON object.
//   key=value ...   model: vocab buckets H dkv dm dff ne nd Lm V own_out (codebooks of their own: 1)   batch: bz Lq L docs
// "dims": the TrainDims; "enc" / "dec": a stack's table, strides and the offsets of every layer; "params": the flat order;
// "index_ok": ParamOrder::index finds every slot at its own position.
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

int main(int argc, char** argv) {
  rpr_model_desc d;
  memset(&d, 0, sizeof d);
  int bz = 1, Lq = 1, L = 1, docs = 2, own_out = 1;
  for (int i = 1; i < argc; ++i) {
    const char* eq = strchr(argv[i], '=');
    if (!eq) { fprintf(stderr, "bad argument %s\n", argv[i]); return 2; }
    const std::string k(argv[i], eq - argv[i]);
    const int v = atoi(eq + 1);
    if (k == "vocab") d.vocab_size = v; else if (k == "buckets") d.rel_buckets = v; else if (k == "H") d.num_heads = v;
    else if (k == "dkv") d.d_kv = v; else if (k == "dm") d.d_model = v; else if (k == "dff") d.d_ff = v;
    else if (k == "ne") d.num_layers = v; else if (k == "nd") d.num_decoder_layers = v; else if (k == "Lm") d.L = v;
    else if (k == "V") d.V = v; else if (k == "own_out") own_out = v; else if (k == "bz") bz = v; else if (k == "Lq") Lq = v;
    else if (k == "L") L = v; else if (k == "docs") docs = v;
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
