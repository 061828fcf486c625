// Tail of the EigenGCN triplet step (Code/eigengcn/tripletnet.py:58-155 on encoders.py:377): pred_model = Linear -> ReLU -> Linear
// on the three graphs' concatenated readouts r[3, D], then both F.pairwise_distance, in ONE launch forward and ONE backward.
//   h[b] = relu(W1 r[b] + b1)  [3, H]      e[b] = W2 h[b] + b2  [3, E]      dist = (||e_a - e_p + eps||, ||e_a - e_n + eps||)
// (A pred_model that is a single Linear is exactly csrc/triplet.hip's tail and goes there.)
//
// Forward: one workgroup of 16 waves.  Phase 1 as triplet_embed_fwd_kernel: a wave takes eight rows of W1 at a time (nn.Linear's
// [out, in] layout, 16-byte loads, eight rows requested together), every W1 row is streamed once for all three readout rows.  Phase 2
// reads h from LDS; W2's rows are H floats long (H = 50 in the reference's default: not 16-byte rows), so its loads are scalar, lanes
// along the row, eight rows together.
// Backward: a grid over slices of 32 input columns; every workgroup re-derives the short chain de[3, E] -> dh[3, H] in LDS (at most
// 3 * 512 * 512 multiply-adds on W2 out of the L2: cheaper than a launch of its own), then owns its columns of dr and dW1 and a
// grid-strided share of dW2; workgroup 0 also writes db1 and db2.
#include "common.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int M2_MAX = 512;          // H, E
constexpr int M2_MAXD = 2048;
constexpr int M2_RPW = 8;            // weight rows per wave and pass

__global__ __launch_bounds__(1024) void mlp2_triplet_fwd_kernel(const float* __restrict__ r, int64_t ldr, const float* __restrict__ w1,
                                                                const float* __restrict__ b1, const float* __restrict__ w2,
                                                                const float* __restrict__ b2, int D, int H, int E, float eps,
                                                                float* __restrict__ h, float* __restrict__ embed, float* __restrict__ dist) {
  __shared__ float hs[3][M2_MAX];
  __shared__ float es[3][M2_MAX];
  __shared__ float red[2][16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int D4 = D >> 2;
  for (int h0 = wid * M2_RPW; h0 < H; h0 += 16 * M2_RPW) {
    float s0[M2_RPW], s1[M2_RPW], s2[M2_RPW];
#pragma unroll
    for (int j = 0; j < M2_RPW; ++j) { s0[j] = 0.f; s1[j] = 0.f; s2[j] = 0.f; }
    for (int c = lane; c < D4; c += 64) {
      float4 wv[M2_RPW];
#pragma unroll
      for (int j = 0; j < M2_RPW; ++j)                                  // rows past H: a mapped row, result dropped
        wv[j] = reinterpret_cast<const float4*>(w1 + (int64_t)min(h0 + j, H - 1) * D)[c];
      const float4 a = reinterpret_cast<const float4*>(r)[c];
      const float4 p = reinterpret_cast<const float4*>(r + ldr)[c];
      const float4 n = reinterpret_cast<const float4*>(r + 2 * ldr)[c];
#pragma unroll
      for (int j = 0; j < M2_RPW; ++j) {
        s0[j] = fmaf(wv[j].x, a.x, fmaf(wv[j].y, a.y, fmaf(wv[j].z, a.z, fmaf(wv[j].w, a.w, s0[j]))));
        s1[j] = fmaf(wv[j].x, p.x, fmaf(wv[j].y, p.y, fmaf(wv[j].z, p.z, fmaf(wv[j].w, p.w, s1[j]))));
        s2[j] = fmaf(wv[j].x, n.x, fmaf(wv[j].y, n.y, fmaf(wv[j].z, n.z, fmaf(wv[j].w, n.w, s2[j]))));
      }
    }
#pragma unroll
    for (int j = 0; j < M2_RPW; ++j) {
      const float t0 = wave_sum(s0[j]), t1 = wave_sum(s1[j]), t2 = wave_sum(s2[j]);
      const int k = h0 + j;
      if (lane == 0 && k < H) {
        const float bias = b1 ? b1[k] : 0.f;
        hs[0][k] = fmaxf(t0 + bias, 0.f); hs[1][k] = fmaxf(t1 + bias, 0.f); hs[2][k] = fmaxf(t2 + bias, 0.f);
      }
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < H; k += 1024) { h[k] = hs[0][k]; h[H + k] = hs[1][k]; h[2 * H + k] = hs[2][k]; }
  for (int e0 = wid * M2_RPW; e0 < E; e0 += 16 * M2_RPW) {
    float s0[M2_RPW], s1[M2_RPW], s2[M2_RPW];
#pragma unroll
    for (int j = 0; j < M2_RPW; ++j) { s0[j] = 0.f; s1[j] = 0.f; s2[j] = 0.f; }
    for (int c = lane; c < H; c += 64) {
      float wv[M2_RPW];
#pragma unroll
      for (int j = 0; j < M2_RPW; ++j) wv[j] = w2[(int64_t)min(e0 + j, E - 1) * H + c];
      const float a = hs[0][c], p = hs[1][c], n = hs[2][c];
#pragma unroll
      for (int j = 0; j < M2_RPW; ++j) { s0[j] = fmaf(wv[j], a, s0[j]); s1[j] = fmaf(wv[j], p, s1[j]); s2[j] = fmaf(wv[j], n, s2[j]); }
    }
#pragma unroll
    for (int j = 0; j < M2_RPW; ++j) {
      const float t0 = wave_sum(s0[j]), t1 = wave_sum(s1[j]), t2 = wave_sum(s2[j]);
      const int e = e0 + j;
      if (lane == 0 && e < E) {
        const float bias = b2 ? b2[e] : 0.f;
        es[0][e] = t0 + bias; es[1][e] = t1 + bias; es[2][e] = t2 + bias;
      }
    }
  }
  __syncthreads();
  float qp = 0.f, qn = 0.f;
  for (int e = threadIdx.x; e < E; e += 1024) {
    embed[e] = es[0][e]; embed[E + e] = es[1][e]; embed[2 * E + e] = es[2][e];
    const float dp = es[0][e] - es[1][e] + eps, dn = es[0][e] - es[2][e] + eps;
    qp = fmaf(dp, dp, qp); qn = fmaf(dn, dn, qn);
  }
  qp = wave_sum(qp); qn = wave_sum(qn);
  if (lane == 0) { red[0][wid] = qp; red[1][wid] = qn; }
  __syncthreads();
  if (threadIdx.x < 2) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += red[threadIdx.x][k];
    dist[threadIdx.x] = sqrtf(s);
  }
}

// workgroup = 32 input columns [32 bx, 32 bx + 32); thread (j = tid & 31, k = tid >> 5): column j, hidden rows k, k + 8, ...
__global__ __launch_bounds__(256) void mlp2_triplet_bwd_kernel(const float* __restrict__ r, int64_t ldr, const float* __restrict__ w1,
                                                               const float* __restrict__ w2, const float* __restrict__ h,
                                                               const float* __restrict__ embed, const float* __restrict__ dist, float eps,
                                                               const float* __restrict__ g_dp, const float* __restrict__ g_dn,
                                                               const float* __restrict__ g_ea, const float* __restrict__ g_ep,
                                                               const float* __restrict__ g_en, int D, int H, int E,
                                                               float* __restrict__ dr, int64_t lddr, float* __restrict__ dw1,
                                                               float* __restrict__ db1, float* __restrict__ dw2, float* __restrict__ db2) {
  __shared__ float de[3][M2_MAX];
  __shared__ float dh[3][M2_MAX];
  __shared__ float hs[3][M2_MAX];
  __shared__ float part[3][8][32];
  const int tid = threadIdx.x;
  const float gp = g_dp ? g_dp[0] : 0.f, gn = g_dn ? g_dn[0] : 0.f;
  const float ip = dist[0] > 0.f ? gp / dist[0] : 0.f, in_ = dist[1] > 0.f ? gn / dist[1] : 0.f;   // (torch: 0 at a zero distance)
  for (int e = tid; e < E; e += 256) {
    const float a = embed[e], p = embed[E + e], n = embed[2 * E + e];
    const float tp = (a - p + eps) * ip, tn = (a - n + eps) * in_;
    de[0][e] = tp + tn + (g_ea ? g_ea[e] : 0.f);
    de[1][e] = -tp + (g_ep ? g_ep[e] : 0.f);
    de[2][e] = -tn + (g_en ? g_en[e] : 0.f);
  }
  for (int k = tid; k < H; k += 256) { hs[0][k] = h[k]; hs[1][k] = h[H + k]; hs[2][k] = h[2 * H + k]; }
  __syncthreads();
  // dh[b, k] = (h[b, k] > 0) sum_e de[b, e] W2[e, k]: threads along a row of W2, eight rows requested together
  for (int k = tid; k < H; k += 256) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int e0 = 0; e0 < E; e0 += 8) {
      float wv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) wv[q] = w2[(int64_t)min(e0 + q, E - 1) * H + k];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (e0 + q < E) { s0 = fmaf(de[0][e0 + q], wv[q], s0); s1 = fmaf(de[1][e0 + q], wv[q], s1); s2 = fmaf(de[2][e0 + q], wv[q], s2); }
      }
    }
    dh[0][k] = hs[0][k] > 0.f ? s0 : 0.f;
    dh[1][k] = hs[1][k] > 0.f ? s1 : 0.f;
    dh[2][k] = hs[2][k] > 0.f ? s2 : 0.f;
  }
  __syncthreads();
  const int j = tid & 31, k = tid >> 5;
  const int d = 32 * (int)blockIdx.x + j;
  const bool ok = d < D;
  const float ra = ok ? r[d] : 0.f, rp = ok ? r[ldr + d] : 0.f, rn = ok ? r[2 * ldr + d] : 0.f;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  const int dc = ok ? d : 0;
  for (int k0 = k; k0 < H; k0 += 64) {                               // eight rows of W1 per pass, requested together
    float wv[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) wv[q] = w1[(int64_t)min(k0 + 8 * q, H - 1) * D + dc];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int kk = k0 + 8 * q;
      if (ok && kk < H) {
        const float g0 = dh[0][kk], g1 = dh[1][kk], g2 = dh[2][kk];
        s0 = fmaf(g0, wv[q], s0); s1 = fmaf(g1, wv[q], s1); s2 = fmaf(g2, wv[q], s2);
        dw1[(int64_t)kk * D + d] = fmaf(g0, ra, fmaf(g1, rp, g2 * rn));
      }
    }
  }
  part[0][k][j] = s0; part[1][k][j] = s1; part[2][k][j] = s2;
  __syncthreads();
  if (dr && tid < 96) {
    const int b = tid >> 5, jj = tid & 31, dd = 32 * (int)blockIdx.x + jj;
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) s += part[b][q][jj];
    if (dd < D) dr[(int64_t)b * lddr + dd] = s;
  }
  // this workgroup's share of dW2[e, k] = sum_b de[b, e] h[b, k]
  const int EH = E * H;
  for (int i = (int)blockIdx.x * 256 + tid; i < EH; i += (int)gridDim.x * 256) {
    const int e = i / H, kk = i - e * H;
    dw2[i] = fmaf(de[0][e], hs[0][kk], fmaf(de[1][e], hs[1][kk], de[2][e] * hs[2][kk]));
  }
  if (blockIdx.x == 0) {
    if (db1) for (int kk = tid; kk < H; kk += 256) db1[kk] = (dh[0][kk] + dh[1][kk]) + dh[2][kk];
    if (db2) for (int e = tid; e < E; e += 256) db2[e] = (de[0][e] + de[1][e]) + de[2][e];
  }
}

}  // namespace

extern "C" {

int tsgnn_mlp2_triplet_supported(int D, int H, int E) {
  return D > 0 && H > 0 && E > 0 && D % 4 == 0 && D <= M2_MAXD && H <= M2_MAX && E <= M2_MAX;
}

int tsgnn_mlp2_triplet_fwd_f32(const float* r, int64_t ldr, const float* w1, const float* b1, const float* w2, const float* b2, int D,
                               int H, int E, float eps, float* h, float* embed, float* dist, hipStream_t stream) {
  if (!r || !w1 || !w2 || !h || !embed || !dist || D <= 0 || H <= 0 || E <= 0 || ldr < D) return TSGNN_EINVAL;
  if (!tsgnn_mlp2_triplet_supported(D, H, E) || (ldr % 4) || ((reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(w1)) & 15))
    return TSGNN_EUNSUPPORTED;
  TSGNN_KNAME("mlp2_triplet_fwd_kernel");
  mlp2_triplet_fwd_kernel<<<1, 1024, 0, stream>>>(r, ldr, w1, b1, w2, b2, D, H, E, eps, h, embed, dist);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

int tsgnn_mlp2_triplet_bwd_f32(const float* r, int64_t ldr, const float* w1, const float* w2, const float* h, const float* embed,
                               const float* dist, float eps, const float* g_dp, const float* g_dn, const float* g_ea, const float* g_ep,
                               const float* g_en, int D, int H, int E, float* dr, int64_t lddr, float* dw1, float* db1, float* dw2,
                               float* db2, hipStream_t stream) {
  if (!r || !w1 || !w2 || !h || !embed || !dist || !dw1 || !dw2 || D <= 0 || H <= 0 || E <= 0 || ldr < D || (dr && lddr < D))
    return TSGNN_EINVAL;
  if (!tsgnn_mlp2_triplet_supported(D, H, E)) return TSGNN_EUNSUPPORTED;
  TSGNN_KNAME("mlp2_triplet_bwd_kernel");
  mlp2_triplet_bwd_kernel<<<(unsigned)((D + 31) / 32), 256, 0, stream>>>(r, ldr, w1, w2, h, embed, dist, eps, g_dp, g_dn, g_ea, g_ep, g_en, D, H,
                                                                         E, dr, lddr, dw1, db1, dw2, db2);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
