// Fragment-major copies of weight matrices: the B operand of the bodies that feed the matrix cores straight from global memory
// (sageconv_body.h, rowgemm_body.h BIMG).  One body, two callers: the stand-alone pack launch (tsgnn_sage_conv_pack_f32, sageconv.hip)
// and the pack RIDERS of a training step's first product launch (tsgnn_gather_rowgemm_st_f32, rowgemm.hip), which write the images of
// the hidden layers' weights from the parameters of that very step — no launch of their own, and nothing cached across steps.
#pragma once
#include "common.h"

struct PackSet {
  const float* w; int64_t ldw; int K, N; int kn;        // kn = 0: w[n * ldw + k] (nn.Linear's [out, in]); 1: w[k * ldw + n]
  float4* out;                                          // [4 waves][16 steps][64 lanes]
};
constexpr int PACK_SET_ENTRIES = 4096;                  // float4 per image

// entry e (0 .. 4095) of one image:  out[(wv * 16 + u) * 64 + lane] = W[k = 8u + 4h + 0..3][n = 32 wv + i]  (lane = 32 h + i), zero
// beyond K / N
__device__ __forceinline__ void sage_conv_pack_body(const PackSet& s, int e) {
  const int lane = e & 63, u = (e >> 6) & 15, wv = e >> 10;
  const int i = lane & 31, h = lane >> 5;
  const int n = 32 * wv + i, k0 = 8 * u + 4 * h;
  float v[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k = k0 + c;
    const bool ok = n < s.N && k < s.K;
    v[c] = ok ? (s.kn ? s.w[(int64_t)k * s.ldw + n] : s.w[(int64_t)n * s.ldw + k]) : 0.f;
  }
  s.out[e] = make_float4(v[0], v[1], v[2], v[3]);
}

// host: one descriptor entry (w, ldw, K, N, kn, out) -> PackSet; TSGNN_OK, or the error the pack entry points answer with
static inline int pack_set_from_desc(const int64_t* d, PackSet& s) {
  s.w = reinterpret_cast<const float*>(d[0]); s.ldw = d[1]; s.K = (int)d[2]; s.N = (int)d[3]; s.kn = (int)d[4];
  s.out = reinterpret_cast<float4*>(d[5]);
  if (!s.w || !s.out || s.K < 1 || s.K > 128 || s.N < 1 || s.N > 128 || s.ldw < (s.kn ? s.N : s.K)) return TSGNN_EINVAL;
  if (reinterpret_cast<uintptr_t>(s.out) & 15) return TSGNN_EUNSUPPORTED;
  return TSGNN_OK;
}

// passengers of a carrier launch: workgroup b of `blocks` (of blockDim.x threads) writes blockDim.x entries of image b * blockDim.x / 4096
constexpr int PACK_RIDER_SETS = 8;
struct PackRider { PackSet s[PACK_RIDER_SETS]; unsigned blocks; };    // blocks = 0: none
__device__ __forceinline__ void pack_rider_body(const PackRider& p, unsigned b) {
  const unsigned e = b * blockDim.x + threadIdx.x;
  sage_conv_pack_body(p.s[e / PACK_SET_ENTRIES], (int)(e % PACK_SET_ENTRIES));
}
