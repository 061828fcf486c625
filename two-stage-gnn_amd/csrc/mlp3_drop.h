// The in-launch dropout mask of the SAGPool head (Code/sag/network.py:49), shared by every launch that draws it (csrc/mlp_head.hip:
// tsgnn_mlp3_fwd_drop_f32, tsgnn_mlp3_triplet_fwd_f32, tsgnn_mlp3_dropout_mask_f32; csrc/posttrain_cls.hip: the post-training head), so
// that one seed / counter pair names one mask whichever launch made it.
//
// Element (b, j) of the hidden layer is kept when its 32 Philox bits are >= thresh (= p * 2^32), keyed on (seed + the DEVICE counter
// state[0]; b, j).  The counter advances once per launch, so a training step replayed from a hipGraph draws a new mask at every replay
// without a host-side generator (torch's graph-safe generator costs a bernoulli launch plus two fill launches per replay).
// used[0] = the counter value of this launch (tests regenerate the mask).
#pragma once
#include "common.h"

struct Mlp3Drop {
  unsigned thresh; unsigned seed_lo, seed_hi;
  unsigned long long* state;             // [0] launches so far, [1] tickets of the running launch (zero between launches)
  unsigned long long* used;
};

__device__ __forceinline__ float mlp3_keep(unsigned thresh, unsigned klo, unsigned khi, unsigned b, unsigned j) {
  const uint4 r = philox4x32_10(make_uint4(b, j >> 2, 0u, 0x4D4C5033u), make_uint2(klo, khi));
  const unsigned v = (j & 3) == 0 ? r.x : (j & 3) == 1 ? r.y : (j & 3) == 2 ? r.z : r.w;
  return v < thresh ? 0.f : 1.f;
}

static inline unsigned mlp3_thresh(float p) {
  const double t = (double)p * 4294967296.0;
  return t >= 4294967295.0 ? 0xFFFFFFFFu : (unsigned)t;
}
