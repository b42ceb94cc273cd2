// The dropout mask of the training step: ONE stateless function of (seed, step, site, logical coordinates), evaluated
// wherever a mask is needed — the forward pass and, again, the backward pass (no mask is stored). Restated exactly in numpy
// in tests/dropout_mask.py; DESIGN.md "Dropout in the training step" documents the generator, the sites and the packing.
//
// Generator: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): a 128-bit counter and a
// 64-bit key give four 32-bit draws. An element is DROPPED where its draw is below round(rate * 2^32); a kept element is
// multiplied by fp32(1 / (1 - rate)).
//   key      k0 = seed[31:0]                 k1 = seed[63:32] ^ step[63:32]
//   counter  c1 = sequence                   c3 = step[31:0]
//     activation (sequence, position, feature):        c0 = feature >> 2              c2 = site << 16 | position
//     attention  (sequence, head, query pos, key pos): c0 = query << 16 | key >> 2    c2 = site << 16 | head
//   the element's draw is word (feature & 3) / (key pos & 3) of the block.
// sequence = b in the encoder, b * n_docs + doc in the decoder. Nothing here knows a memory offset, a tile or a lane: the mask
// is the same whatever the launch shape, the precision mode or the padding of a row stride.
// Sites (16 bits): stack << 11 | code, stack = 0 encoder / 1 decoder; code 0 = the stack's input embeddings, 1 = its output
// (after the final norm), 8 + 8 layer + 2 j = the middle of sub-block j (attention probabilities, or the feed-forward's
// relu(h Wi^T)), 8 + 8 layer + 2 j + 1 = the sub-block's output before the residual is added.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define RPR_HD __host__ __device__ __forceinline__
#else
#define RPR_HD inline
#endif

namespace rpr {

struct DropKey {
  uint32_t k0, k1, step_lo, thr;   // thr = round(rate * 2^32): 0 = dropout is off
  float scale;                     // fp32(1 / (1 - rate))
};

// what an attention kernel is handed: the site of its probabilities; L = decoder positions per sequence (cross-attention, whose
// blocks hold all the decoder rows of a query: row r is position r % L of sequence query * n_docs + r / L)
struct DropAttn { DropKey key; int site, L; };

// the key of one pass (host): 0 <= rate < 1, checked by the entry points
inline DropKey drop_key(float rate, uint64_t seed, uint64_t step) {
  DropKey key{};
  key.k0 = (uint32_t)seed; key.k1 = (uint32_t)(seed >> 32) ^ (uint32_t)(step >> 32); key.step_lo = (uint32_t)step;
  key.thr = (uint32_t)llrint((double)rate * 4294967296.0);
  key.scale = 1.0f / (1.0f - rate);
  return key;
}
inline DropAttn drop_attn(const DropKey& key, int site, int L) { return DropAttn{key, site, L}; }

RPR_HD int drop_site(int dec, int code) { return (dec << 11) | code; }
RPR_HD int drop_site_input(int dec) { return drop_site(dec, 0); }
RPR_HD int drop_site_output(int dec) { return drop_site(dec, 1); }
RPR_HD int drop_site_mid(int dec, int layer, int j) { return drop_site(dec, 8 + 8 * layer + 2 * j); }
RPR_HD int drop_site_sub_out(int dec, int layer, int j) { return drop_site(dec, 8 + 8 * layer + 2 * j + 1); }

struct Draw4 { uint32_t w[4]; };

RPR_HD Draw4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Draw4{{c0, c1, c2, c3}};
}

// the four draws of features 4 q .. 4 q + 3 of an activation row
RPR_HD Draw4 drop_draws_act(const DropKey& k, int site, uint32_t seq, int pos, int q) {
  return philox4x32_10((uint32_t)q, seq, ((uint32_t)site << 16) | (uint32_t)pos, k.step_lo, k.k0, k.k1);
}
// the attention probabilities of keys 4 g .. 4 g + 3 of one query row: bit k set = key 4 g + k is KEPT (one Philox block)
RPR_HD uint32_t drop_keep4_attn(const DropKey& k, int site, uint32_t seq, int head, int qpos, int g) {
  const Draw4 d = philox4x32_10(((uint32_t)qpos << 16) | (uint32_t)g, seq, ((uint32_t)site << 16) | (uint32_t)head, k.step_lo, k.k0, k.k1);
  return (d.w[0] >= k.thr ? 1u : 0u) | (d.w[1] >= k.thr ? 2u : 0u) | (d.w[2] >= k.thr ? 4u : 0u) | (d.w[3] >= k.thr ? 8u : 0u);
}

}  // namespace rpr
