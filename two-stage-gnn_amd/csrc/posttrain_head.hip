// Head of the 2stg+ post-training step (Code/sage+gat+diffpool/train_triplet_pre_train.py:196-270): on the readout rows r[R, P] of the
// step's graphs (R = 1 in the reference's loop, up to 8 here)
//   out = r W0^T + b0            [R, E]     map_model
//   z1 = out W1^T + b1, z2 = leaky(z1) W2^T + b2, z = leaky(z2) W3^T + b3    the replacement map2_model, z = the reference's `pred`
//   p = softmax(z);  loss_i = logsumexp(p_i) - p_i[label_i];  loss = mean_i loss_i       (:256: F.cross_entropy(F.softmax(pred), label),
//                                                                                         the softmax applied twice, kept literally)
// with label_i = labels[ids[i]] read on the device (ids: what the gather launch of the stream wrote), in ONE launch forward and ONE
// backward.
//
// Forward: one workgroup of 16 waves.  map_model as mlp2_triplet_fwd_kernel does it: a wave takes a few rows of W0 at a time, 16-byte
// loads, every W0 row streamed once for all R readout rows.  The three small layers: a wave per output unit, lanes along the unit's
// weight row (rows of E, h1, h2 floats: not 16-byte rows in general), the inputs an LDS read.  Soft-max and loss: one thread per row,
// classes in order.
// Backward: a grid over slices of 32 columns of r; every workgroup re-derives the short chain dz -> dz2 -> dz1 -> dout[R, E] in LDS
// (at most 8 * 64 * 512 multiply-adds on W1 out of the L2: cheaper than a launch of its own), then owns its columns of dr and dW0 and
// a grid-strided share of the three small weight gradients and the four bias gradients.  Every output element is written once, every
// sum runs in a fixed order (rows 0 .. R - 1, classes 0 .. C - 1, the eight partial sums of a column in order): two runs give the same
// bits.  Rows R .. RT - 1 of the LDS tiles hold zeros, so the row loops have a compile-time length and the accumulators stay in
// registers (no private segment in any variant: -Rpass-analysis=kernel-resource-usage).
#include "common.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int PT_MAXP = 2048, PT_MAXE = 512, PT_MAXH = 64, PT_MAXC = 64, PT_MAXR = 8;

struct PtFwd {
  const float* r;
  int64_t ldr;
  const float *w0, *b0, *w1, *b1, *w2, *b2, *w3, *b3;
  const int *ids, *labels;
  int n_labels, R, P, E, h1, h2, C;
  float slope;
  float *out, *z1, *z2, *z, *p, *loss;
};

struct PtBwd {
  const float* r;
  int64_t ldr;
  const float *w0, *w1, *w2, *w3, *out, *z1, *z2, *p;
  const int *ids, *labels;
  const float* g;
  int n_labels, R, P, E, h1, h2, C;
  float slope;
  float* dr;
  int64_t lddr;
  float *dw0, *db0, *dw1, *db1, *dw2, *db2, *dw3, *db3;
};

__device__ __forceinline__ float pt_leaky(float v, float slope) { return v > 0.f ? v : slope * v; }
__device__ __forceinline__ float pt_leaky_grad(float v, float slope) { return v > 0.f ? 1.f : slope; }   // at exactly 0: slope (torch)

// label of row i: labels[ids[i]], both clamped into their tables (the host validates what it can see; these live on the device)
__device__ __forceinline__ int pt_label(const int* ids, const int* labels, int n_labels, int C, int i) {
  const int id = min(max(ids[i], 0), n_labels - 1);
  return min(max(labels[id], 0), C - 1);
}

// one small layer for all rows: a wave per output unit n, lanes along the unit's K weights; pre-activations to memory, the
// (activated) values to the LDS tile of the next layer
template <int RT>
__device__ __forceinline__ void pt_small_layer(const float* __restrict__ w, const float* __restrict__ b, int K, int N, int R,
                                               const float* in, int ldin, float slope, bool act, float* __restrict__ zg, float* aout) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int n = wid; n < N; n += 16) {
    float s[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) s[i] = 0.f;
    for (int k = lane; k < K; k += 64) {
      const float wv = w[(int64_t)n * K + k];
#pragma unroll
      for (int i = 0; i < RT; ++i) s[i] = fmaf(wv, in[i * ldin + k], s[i]);
    }
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const float t = wave_sum(s[i]);
      if (lane == 0 && i < R) {
        const float v = t + b[n];
        zg[i * N + n] = v;
        aout[i * PT_MAXH + n] = act ? pt_leaky(v, slope) : v;
      }
    }
  }
}

template <int RT>
__global__ __launch_bounds__(1024) void posttrain_head_fwd_kernel(const PtFwd a) {
  __shared__ float outs[RT][PT_MAXE];
  __shared__ float act1[RT][PT_MAXH], act2[RT][PT_MAXH], zs[RT][PT_MAXH];
  __shared__ float li[PT_MAXR];
  constexpr int RPW = RT <= 2 ? 8 : 4;                                  // rows of W0 per wave and pass
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int R = a.R, P = a.P, E = a.E, h1 = a.h1, h2 = a.h2, C = a.C;
  const int P4 = P >> 2;
  for (int j = threadIdx.x; j < RT * PT_MAXE; j += 1024) (&outs[0][0])[j] = 0.f;      // (rows R .. RT - 1 are read by the layers below)
  for (int j = threadIdx.x; j < RT * PT_MAXH; j += 1024) (&act1[0][0])[j] = (&act2[0][0])[j] = 0.f;
  __syncthreads();
  for (int e0 = wid * RPW; e0 < E; e0 += 16 * RPW) {
    float s[RPW][RT];
#pragma unroll
    for (int j = 0; j < RPW; ++j)
#pragma unroll
      for (int i = 0; i < RT; ++i) s[j][i] = 0.f;
    for (int c = lane; c < P4; c += 64) {
      float4 wv[RPW];
#pragma unroll
      for (int j = 0; j < RPW; ++j)                                      // rows past E: a mapped row, result dropped
        wv[j] = reinterpret_cast<const float4*>(a.w0 + (int64_t)min(e0 + j, E - 1) * P)[c];
#pragma unroll
      for (int i = 0; i < RT; ++i) {                                     // rows past R: the last row again, result dropped
        const float4 rv = reinterpret_cast<const float4*>(a.r + (int64_t)min(i, R - 1) * a.ldr)[c];
#pragma unroll
        for (int j = 0; j < RPW; ++j)
          s[j][i] = fmaf(wv[j].x, rv.x, fmaf(wv[j].y, rv.y, fmaf(wv[j].z, rv.z, fmaf(wv[j].w, rv.w, s[j][i]))));
      }
    }
#pragma unroll
    for (int j = 0; j < RPW; ++j)
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        const float t = wave_sum(s[j][i]);
        const int e = e0 + j;
        if (lane == 0 && e < E && i < R) {
          const float v = t + a.b0[e];
          outs[i][e] = v;
          a.out[i * E + e] = v;
        }
      }
  }
  __syncthreads();
  pt_small_layer<RT>(a.w1, a.b1, E, h1, R, &outs[0][0], PT_MAXE, a.slope, true, a.z1, &act1[0][0]);
  __syncthreads();
  pt_small_layer<RT>(a.w2, a.b2, h1, h2, R, &act1[0][0], PT_MAXH, a.slope, true, a.z2, &act2[0][0]);
  __syncthreads();
  pt_small_layer<RT>(a.w3, a.b3, h2, C, R, &act2[0][0], PT_MAXH, a.slope, false, a.z, &zs[0][0]);
  __syncthreads();
  if (threadIdx.x < R) {
    const int i = threadIdx.x;
    float* const zi = zs[i];
    float m = zi[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, zi[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) {
      const float e = expf(zi[c] - m);
      zi[c] = e;
      se += e;
    }
    const float inv = 1.f / se;
    float pm = 0.f;
    for (int c = 0; c < C; ++c) {
      const float pv = zi[c] * inv;
      zi[c] = pv;
      a.p[i * C + c] = pv;
      pm = fmaxf(pm, pv);
    }
    float sp = 0.f;
    for (int c = 0; c < C; ++c) sp += expf(zi[c] - pm);
    li[i] = (pm + logf(sp)) - zi[pt_label(a.ids, a.labels, a.n_labels, C, i)];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < R; ++i) s += li[i];
    a.loss[0] = s / (float)R;
  }
}

// workgroup = 32 columns [32 bx, 32 bx + 32) of r; thread (j = tid & 31, k = tid >> 5): column j, rows k, k + 8, ... of W0
template <int RT>
__global__ __launch_bounds__(256) void posttrain_head_bwd_kernel(const PtBwd a) {
  __shared__ float outs[RT][PT_MAXE];
  __shared__ float douts[RT][PT_MAXE];
  __shared__ float dzs[RT][PT_MAXC], dz2s[RT][PT_MAXH], dz1s[RT][PT_MAXH], z1s[RT][PT_MAXH], z2s[RT][PT_MAXH];
  __shared__ float part[RT][8][32];
  const int tid = threadIdx.x;
  const int R = a.R, P = a.P, E = a.E, h1 = a.h1, h2 = a.h2, C = a.C;
  const float slope = a.slope;
  for (int idx = tid; idx < RT * E; idx += 256) {
    const int i = idx / E, e = idx - i * E;
    outs[i][e] = i < R ? a.out[idx] : 0.f;
  }
  for (int idx = tid; idx < RT * h1; idx += 256) {
    const int i = idx / h1, j = idx - i * h1;
    z1s[i][j] = i < R ? a.z1[idx] : 0.f;
  }
  for (int idx = tid; idx < RT * h2; idx += 256) {
    const int i = idx / h2, k = idx - i * h2;
    z2s[i][k] = i < R ? a.z2[idx] : 0.f;
  }
  // dz of row i: dp = g (softmax(p) - onehot) / R, the true class as minus the others' sum (no cancellation against 1), then the
  // soft-max backward dz_j = p_j (dp_j - sum_k p_k dp_k); classes in order
  if (tid < RT) {
    const int i = tid;
    float* const d = dzs[i];
    if (i < R) {
      const float* const pi = a.p + i * C;
      const int y = pt_label(a.ids, a.labels, a.n_labels, C, i);
      const float scale = (a.g ? a.g[0] : 1.f) / (float)R;
      float pm = 0.f;
      for (int c = 0; c < C; ++c) pm = fmaxf(pm, pi[c]);
      float so = 0.f;
      for (int c = 0; c < C; ++c) {
        const float e = expf(pi[c] - pm);
        d[c] = e;
        so += c == y ? 0.f : e;
      }
      const float inv = scale / (d[y] + so);
      float dot = 0.f;
      for (int c = 0; c < C; ++c) {
        const float dp = (c == y ? -so : d[c]) * inv;
        d[c] = dp;
        dot = fmaf(pi[c], dp, dot);
      }
      for (int c = 0; c < C; ++c) d[c] = pi[c] * (d[c] - dot);
    } else {
      for (int c = 0; c < C; ++c) d[c] = 0.f;
    }
  }
  __syncthreads();
  for (int idx = tid; idx < RT * h2; idx += 256) {                     // dz2 = (dz W3) * leaky'(z2): threads along a row of W3
    const int i = idx / h2, k = idx - i * h2;
    float s = 0.f;
    for (int c = 0; c < C; ++c) s = fmaf(dzs[i][c], a.w3[c * h2 + k], s);
    dz2s[i][k] = s * pt_leaky_grad(z2s[i][k], slope);
  }
  __syncthreads();
  for (int idx = tid; idx < RT * h1; idx += 256) {                     // dz1 = (dz2 W2) * leaky'(z1)
    const int i = idx / h1, j = idx - i * h1;
    float s = 0.f;
    for (int k = 0; k < h2; ++k) s = fmaf(dz2s[i][k], a.w2[k * h1 + j], s);
    dz1s[i][j] = s * pt_leaky_grad(z1s[i][j], slope);
  }
  __syncthreads();
  for (int e = tid; e < E; e += 256) {                                 // dout = dz1 W1: threads along a row of W1
    float s[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) s[i] = 0.f;
    for (int j = 0; j < h1; ++j) {
      const float wv = a.w1[j * E + e];
#pragma unroll
      for (int i = 0; i < RT; ++i) s[i] = fmaf(dz1s[i][j], wv, s[i]);
    }
#pragma unroll
    for (int i = 0; i < RT; ++i) douts[i][e] = s[i];
  }
  __syncthreads();
  {
    const int j = tid & 31, k = tid >> 5;
    const int d = 32 * (int)blockIdx.x + j;
    const bool ok = d < P;
    const int dc = ok ? d : 0;
    float rv[RT], acc[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      rv[i] = (ok && i < R) ? a.r[(int64_t)i * a.ldr + d] : 0.f;
      acc[i] = 0.f;
    }
    for (int e0 = k; e0 < E; e0 += 64) {                               // eight rows of W0 per pass, requested together
      float wv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) wv[q] = a.w0[(int64_t)min(e0 + 8 * q, E - 1) * P + dc];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int e = e0 + 8 * q;
        if (ok && e < E) {
          float dw = 0.f;
#pragma unroll
          for (int i = 0; i < RT; ++i) {
            const float gi = douts[i][e];
            acc[i] = fmaf(gi, wv[q], acc[i]);
            dw = fmaf(gi, rv[i], dw);
          }
          a.dw0[(int64_t)e * P + d] = dw;
        }
      }
    }
#pragma unroll
    for (int i = 0; i < RT; ++i) part[i][k][j] = acc[i];
  }
  __syncthreads();
  if (a.dr && tid < RT * 32) {
    const int i = tid >> 5, jj = tid & 31, dd = 32 * (int)blockIdx.x + jj;
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) s += part[i][q][jj];
    if (i < R && dd < P) a.dr[(int64_t)i * a.lddr + dd] = s;
  }
  // this workgroup's share of the small gradients: dW1 | dW2 | dW3 | db0 | db1 | db2 | db3 as one index range
  const int n1 = h1 * E, n2 = n1 + h2 * h1, n3 = n2 + C * h2, n4 = n3 + E, n5 = n4 + h1, n6 = n5 + h2, n7 = n6 + C;
  for (int idx = (int)blockIdx.x * 256 + tid; idx < n7; idx += (int)gridDim.x * 256) {
    float s = 0.f;
    if (idx < n1) {
      const int j = idx / E, e = idx - j * E;
#pragma unroll
      for (int i = 0; i < RT; ++i) s = fmaf(dz1s[i][j], outs[i][e], s);
      a.dw1[idx] = s;
    } else if (idx < n2) {
      const int t = idx - n1, k = t / h1, j = t - k * h1;
#pragma unroll
      for (int i = 0; i < RT; ++i) s = fmaf(dz2s[i][k], pt_leaky(z1s[i][j], slope), s);
      a.dw2[t] = s;
    } else if (idx < n3) {
      const int t = idx - n2, c = t / h2, k = t - c * h2;
#pragma unroll
      for (int i = 0; i < RT; ++i) s = fmaf(dzs[i][c], pt_leaky(z2s[i][k], slope), s);
      a.dw3[t] = s;
    } else if (idx < n4) {
#pragma unroll
      for (int i = 0; i < RT; ++i) s += douts[i][idx - n3];
      a.db0[idx - n3] = s;
    } else if (idx < n5) {
#pragma unroll
      for (int i = 0; i < RT; ++i) s += dz1s[i][idx - n4];
      a.db1[idx - n4] = s;
    } else if (idx < n6) {
#pragma unroll
      for (int i = 0; i < RT; ++i) s += dz2s[i][idx - n5];
      a.db2[idx - n5] = s;
    } else {
#pragma unroll
      for (int i = 0; i < RT; ++i) s += dzs[i][idx - n6];
      a.db3[idx - n6] = s;
    }
  }
}

// The loss alone, on rows that ARE the step's `pred` (DGATEncoderGraph with final_dim 'output_dim' returns the readout row first,
// encoders_GAT.py:189-198, so train_triplet_pre_train.py:256 takes both soft-maxes over its embedding_dim columns): one wave, lanes
// along the C <= 1024 columns, rows in order; every sum is a DPP wave sum of per-lane partial sums taken in column order, so two runs
// give the same bits.
struct PtRowLoss {
  const float* z;
  int64_t ldz;
  const int *ids, *labels;
  int n_labels, R, C;
  float *p, *loss;
};

struct PtRowLossBwd {
  const float* p;
  const int *ids, *labels;
  const float* g;
  int n_labels, R, C;
  float* dz;
  int64_t lddz;
};

constexpr int PT_ROW_MAXC = 1024;

__global__ __launch_bounds__(64) void posttrain_rowloss_fwd_kernel(const PtRowLoss a) {
  const int lane = threadIdx.x, C = a.C;
  float total = 0.f;
  for (int i = 0; i < a.R; ++i) {
    const float* const zi = a.z + (int64_t)i * a.ldz;
    float m = -INFINITY;
    for (int c = lane; c < C; c += 64) m = fmaxf(m, zi[c]);
    m = wave_max(m);
    float se = 0.f;
    for (int c = lane; c < C; c += 64) se += expf(zi[c] - m);
    const float inv = 1.f / wave_sum(se);
    float pm = 0.f;
    for (int c = lane; c < C; c += 64) {
      const float pv = expf(zi[c] - m) * inv;
      a.p[i * C + c] = pv;
      pm = fmaxf(pm, pv);
    }
    pm = wave_max(pm);
    float sp = 0.f;
    for (int c = lane; c < C; c += 64) sp += expf(expf(zi[c] - m) * inv - pm);
    sp = wave_sum(sp);
    const int y = pt_label(a.ids, a.labels, a.n_labels, C, i);
    total += (pm + logf(sp)) - expf(zi[y] - m) * inv;
  }
  if (lane == 0) a.loss[0] = total / (float)a.R;
}

// dp = g (softmax(p) - onehot) / R with the true class as minus the others' sum, then dz_c = p_c (dp_c - sum_k p_k dp_k): what
// posttrain_head_bwd_kernel does for its logits
__global__ __launch_bounds__(64) void posttrain_rowloss_bwd_kernel(const PtRowLossBwd a) {
  const int lane = threadIdx.x, C = a.C;
  const float scale = (a.g ? a.g[0] : 1.f) / (float)a.R;
  for (int i = 0; i < a.R; ++i) {
    const float* const pi = a.p + i * C;
    const int y = pt_label(a.ids, a.labels, a.n_labels, C, i);
    float pm = 0.f;
    for (int c = lane; c < C; c += 64) pm = fmaxf(pm, pi[c]);
    pm = wave_max(pm);
    float so = 0.f;
    for (int c = lane; c < C; c += 64) so += c == y ? 0.f : expf(pi[c] - pm);
    so = wave_sum(so);
    const float inv = scale / (expf(pi[y] - pm) + so);
    float dot = 0.f;
    for (int c = lane; c < C; c += 64) dot = fmaf(pi[c], (c == y ? -so : expf(pi[c] - pm)) * inv, dot);
    dot = wave_sum(dot);
    for (int c = lane; c < C; c += 64) a.dz[(int64_t)i * a.lddz + c] = pi[c] * ((c == y ? -so : expf(pi[c] - pm)) * inv - dot);
  }
}

bool pt_dims_ok(int P, int E, int h1, int h2, int C, int R) {
  return P >= 4 && P % 4 == 0 && P <= PT_MAXP && E >= 1 && E <= PT_MAXE && h1 >= 1 && h1 <= PT_MAXH && h2 >= 1 && h2 <= PT_MAXH && C >= 2 &&
         C <= PT_MAXC && R >= 1 && R <= PT_MAXR;
}

}  // namespace

extern "C" {

int tsgnn_posttrain_head_supported(int P, int E, int h1, int h2, int C, int R) { return pt_dims_ok(P, E, h1, h2, C, R) ? 1 : 0; }

#define TSGNN_PT_DISPATCH(KERNEL, GRID, BLOCK)                                   \
  do {                                                                           \
    const int rt = R <= 1 ? 1 : R <= 2 ? 2 : R <= 4 ? 4 : 8;                     \
    TSGNN_KNAME(#KERNEL "<%d>", rt);                                             \
    if (rt == 1) KERNEL<1><<<GRID, BLOCK, 0, stream>>>(a);                       \
    else if (rt == 2) KERNEL<2><<<GRID, BLOCK, 0, stream>>>(a);                  \
    else if (rt == 4) KERNEL<4><<<GRID, BLOCK, 0, stream>>>(a);                  \
    else KERNEL<8><<<GRID, BLOCK, 0, stream>>>(a);                               \
  } while (0)

int tsgnn_posttrain_head_fwd_f32(const float* r, int64_t ldr, int R, int P, const float* w0, const float* b0, int E, const float* w1,
                                 const float* b1, int h1, const float* w2, const float* b2, int h2, const float* w3, const float* b3, int C,
                                 float negative_slope, const int32_t* ids, const int32_t* labels, int64_t n_labels, float* out, float* z1,
                                 float* z2, float* z, float* p, float* loss, hipStream_t stream) {
  if (!r || !w0 || !b0 || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !ids || !labels || !out || !z1 || !z2 || !z || !p || !loss ||
      n_labels < 1 || n_labels > 0x7fffffff || R < 1 || R > PT_MAXR || P < 1 || E < 1 || h1 < 1 || h2 < 1 || C < 2 || ldr < P)
    return TSGNN_EINVAL;
  if (!pt_dims_ok(P, E, h1, h2, C, R) || (ldr % 4) || ((reinterpret_cast<uintptr_t>(r) | reinterpret_cast<uintptr_t>(w0)) & 15))
    return TSGNN_EUNSUPPORTED;
  PtFwd a;
  a.r = r; a.ldr = ldr;
  a.w0 = w0; a.b0 = b0; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.w3 = w3; a.b3 = b3;
  a.ids = ids; a.labels = labels; a.n_labels = (int)n_labels;
  a.R = R; a.P = P; a.E = E; a.h1 = h1; a.h2 = h2; a.C = C;
  a.slope = negative_slope;
  a.out = out; a.z1 = z1; a.z2 = z2; a.z = z; a.p = p; a.loss = loss;
  TSGNN_PT_DISPATCH(posttrain_head_fwd_kernel, 1, 1024);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

int tsgnn_posttrain_head_bwd_f32(const float* r, int64_t ldr, int R, int P, const float* w0, int E, const float* w1, int h1, const float* w2,
                                 int h2, const float* w3, int C, float negative_slope, const int32_t* ids, const int32_t* labels,
                                 int64_t n_labels, const float* out, const float* z1, const float* z2, const float* p, const float* g_loss,
                                 float* dr, int64_t lddr, float* dw0, float* db0, float* dw1, float* db1, float* dw2, float* db2, float* dw3,
                                 float* db3, hipStream_t stream) {
  if (!r || !w0 || !w1 || !w2 || !w3 || !ids || !labels || !out || !z1 || !z2 || !p || !dw0 || !db0 || !dw1 || !db1 || !dw2 || !db2 ||
      !dw3 || !db3 || n_labels < 1 || n_labels > 0x7fffffff || R < 1 || R > PT_MAXR || P < 1 || E < 1 || h1 < 1 || h2 < 1 || C < 2 ||
      ldr < P || (dr && lddr < P))
    return TSGNN_EINVAL;
  if (!pt_dims_ok(P, E, h1, h2, C, R)) return TSGNN_EUNSUPPORTED;
  PtBwd a;
  a.r = r; a.ldr = ldr;
  a.w0 = w0; a.w1 = w1; a.w2 = w2; a.w3 = w3; a.out = out; a.z1 = z1; a.z2 = z2; a.p = p;
  a.ids = ids; a.labels = labels; a.g = g_loss; a.n_labels = (int)n_labels;
  a.R = R; a.P = P; a.E = E; a.h1 = h1; a.h2 = h2; a.C = C;
  a.slope = negative_slope;
  a.dr = dr; a.lddr = lddr;
  a.dw0 = dw0; a.db0 = db0; a.dw1 = dw1; a.db1 = db1; a.dw2 = dw2; a.db2 = db2; a.dw3 = dw3; a.db3 = db3;
  TSGNN_PT_DISPATCH(posttrain_head_bwd_kernel, (unsigned)((P + 31) / 32), 256);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

#undef TSGNN_PT_DISPATCH

int tsgnn_posttrain_rowloss_supported(int C, int R) { return (C >= 2 && C <= PT_ROW_MAXC && R >= 1 && R <= PT_MAXR) ? 1 : 0; }

int tsgnn_posttrain_rowloss_fwd_f32(const float* z, int64_t ldz, int R, int C, const int32_t* ids, const int32_t* labels, int64_t n_labels,
                                    float* p, float* loss, hipStream_t stream) {
  if (!z || !ids || !labels || !p || !loss || n_labels < 1 || n_labels > 0x7fffffff || R < 1 || C < 2 || ldz < C) return TSGNN_EINVAL;
  if (!tsgnn_posttrain_rowloss_supported(C, R)) return TSGNN_EUNSUPPORTED;
  PtRowLoss a;
  a.z = z; a.ldz = ldz; a.ids = ids; a.labels = labels; a.n_labels = (int)n_labels; a.R = R; a.C = C; a.p = p; a.loss = loss;
  TSGNN_KNAME("posttrain_rowloss_fwd_kernel");
  posttrain_rowloss_fwd_kernel<<<1, 64, 0, stream>>>(a);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

int tsgnn_posttrain_rowloss_bwd_f32(const float* p, int R, int C, const int32_t* ids, const int32_t* labels, int64_t n_labels,
                                    const float* g_loss, float* dz, int64_t lddz, hipStream_t stream) {
  if (!p || !ids || !labels || !dz || n_labels < 1 || n_labels > 0x7fffffff || R < 1 || C < 2 || lddz < C) return TSGNN_EINVAL;
  if (!tsgnn_posttrain_rowloss_supported(C, R)) return TSGNN_EUNSUPPORTED;
  PtRowLossBwd a;
  a.p = p; a.ids = ids; a.labels = labels; a.g = g_loss; a.n_labels = (int)n_labels; a.R = R; a.C = C; a.dz = dz; a.lddz = lddz;
  TSGNN_KNAME("posttrain_rowloss_bwd_kernel");
  posttrain_rowloss_bwd_kernel<<<1, 64, 0, stream>>>(a);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
