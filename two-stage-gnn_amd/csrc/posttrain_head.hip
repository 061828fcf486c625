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
// bits.  Rows R .. RT - 1 of the LDS tiles hold zeros (backward) or what row R - 1 gives, never stored to memory (forward), so the
// row loops have a compile-time length and the accumulators stay in registers (no private segment in any variant:
// -Rpass-analysis=kernel-resource-usage).
// map_model's layer, the three small layers and the backward's block of 32 columns are csrc/head_rows_body.h's rows_dense16,
// rows_dense1 (one weight row per wave) and rows_input_columns; the soft-max taken twice, the chain through the leaky layers and the
// index range of the small gradients are this head's own.
#include "common.h"
#include "head_rows_body.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int PT_MAXP = 2048, PT_MAXE = 512, PT_MAXH = 64, PT_MAXC = 64;

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

__device__ __forceinline__ float pt_leaky_grad(float v, float slope) { return v > 0.f ? 1.f : slope; }   // at exactly 0: slope (torch)

template <int RT>
__global__ __launch_bounds__(1024) void posttrain_head_fwd_kernel(const PtFwd a) {
  __shared__ float outs[RT][PT_MAXE];
  __shared__ float act1[RT][PT_MAXH], act2[RT][PT_MAXH], zs[RT][PT_MAXH];
  __shared__ float li[ROWS_MAXR];
  constexpr int RPW = RT <= 2 ? 8 : 4;                                  // rows of W0 per wave and pass
  const int R = a.R, P = a.P, E = a.E, h1 = a.h1, h2 = a.h2, C = a.C;
  for (int j = threadIdx.x; j < RT * PT_MAXE; j += 1024) (&outs[0][0])[j] = 0.f;      // (every word of the tiles is read by the layers below)
  for (int j = threadIdx.x; j < RT * PT_MAXH; j += 1024) (&act1[0][0])[j] = (&act2[0][0])[j] = 0.f;
  __syncthreads();
  rows_dense16<RT, RPW, 16, false>(a.r, a.ldr, R, P, a.w0, P, a.b0, E, &outs[0][0], PT_MAXE, a.out, R);
  __syncthreads();
  // the three small layers: a wave per output unit, lanes along the unit's weight row
  rows_dense1<RT, 1, 16>(&outs[0][0], PT_MAXE, E, a.w1, a.b1, h1, R, true, a.slope, a.z1, &act1[0][0], PT_MAXH);
  __syncthreads();
  rows_dense1<RT, 1, 16>(&act1[0][0], PT_MAXH, h1, a.w2, a.b2, h2, R, true, a.slope, a.z2, &act2[0][0], PT_MAXH);
  __syncthreads();
  rows_dense1<RT, 1, 16>(&act2[0][0], PT_MAXH, h2, a.w3, a.b3, C, R, false, a.slope, a.z, &zs[0][0], PT_MAXH);
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
    li[i] = (pm + logf(sp)) - zi[row_label(a.ids, a.labels, a.n_labels, C, i)];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int i = 0; i < R; ++i) s += li[i];
    a.loss[0] = s / (float)R;
  }
}

template <int RT>
__global__ __launch_bounds__(256) void posttrain_head_bwd_kernel(const PtBwd a) {
  __shared__ float outs[RT][PT_MAXE];
  __shared__ float douts[RT * PT_MAXE];      // [RT][E]
  __shared__ float dzs[RT][PT_MAXC], dz2s[RT][PT_MAXH], dz1s[RT][PT_MAXH], z1s[RT][PT_MAXH], z2s[RT][PT_MAXH];
  __shared__ float part[RT * 256];
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
      const int y = row_label(a.ids, a.labels, a.n_labels, C, i);
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
    for (int i = 0; i < RT; ++i) douts[i * E + e] = s[i];
  }
  __syncthreads();
  rows_input_columns<RT, 256>(a.r, a.ldr, R, P, a.w0, P, E, douts, a.dr, a.lddr, a.dw0, P, part);
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
      for (int i = 0; i < RT; ++i) s = fmaf(dz2s[i][k], rows_leaky(z1s[i][j], slope), s);
      a.dw2[t] = s;
    } else if (idx < n3) {
      const int t = idx - n2, c = t / h2, k = t - c * h2;
#pragma unroll
      for (int i = 0; i < RT; ++i) s = fmaf(dzs[i][c], rows_leaky(z2s[i][k], slope), s);
      a.dw3[t] = s;
    } else if (idx < n4) {
#pragma unroll
      for (int i = 0; i < RT; ++i) s += douts[i * E + idx - n3];
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
    const int y = row_label(a.ids, a.labels, a.n_labels, C, i);
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
    const int y = row_label(a.ids, a.labels, a.n_labels, C, i);
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
         C <= PT_MAXC && R >= 1 && R <= ROWS_MAXR;
}

}  // namespace

extern "C" {

int tsgnn_posttrain_head_supported(int P, int E, int h1, int h2, int C, int R) { return pt_dims_ok(P, E, h1, h2, C, R) ? 1 : 0; }

int tsgnn_posttrain_head_fwd_f32(const float* r, int64_t ldr, int R, int P, const float* w0, const float* b0, int E, const float* w1,
                                 const float* b1, int h1, const float* w2, const float* b2, int h2, const float* w3, const float* b3, int C,
                                 float negative_slope, const int32_t* ids, const int32_t* labels, int64_t n_labels, float* out, float* z1,
                                 float* z2, float* z, float* p, float* loss, hipStream_t stream) {
  if (!r || !w0 || !b0 || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !ids || !labels || !out || !z1 || !z2 || !z || !p || !loss ||
      n_labels < 1 || n_labels > 0x7fffffff || R < 1 || R > ROWS_MAXR || P < 1 || E < 1 || h1 < 1 || h2 < 1 || C < 2 || ldr < P)
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
  TSGNN_ROWS_DISPATCH(posttrain_head_fwd_kernel, R, 1, 1024, 0);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

int tsgnn_posttrain_head_bwd_f32(const float* r, int64_t ldr, int R, int P, const float* w0, int E, const float* w1, int h1, const float* w2,
                                 int h2, const float* w3, int C, float negative_slope, const int32_t* ids, const int32_t* labels,
                                 int64_t n_labels, const float* out, const float* z1, const float* z2, const float* p, const float* g_loss,
                                 float* dr, int64_t lddr, float* dw0, float* db0, float* dw1, float* db1, float* dw2, float* db2, float* dw3,
                                 float* db3, hipStream_t stream) {
  if (!r || !w0 || !w1 || !w2 || !w3 || !ids || !labels || !out || !z1 || !z2 || !p || !dw0 || !db0 || !dw1 || !db1 || !dw2 || !db2 ||
      !dw3 || !db3 || n_labels < 1 || n_labels > 0x7fffffff || R < 1 || R > ROWS_MAXR || P < 1 || E < 1 || h1 < 1 || h2 < 1 || C < 2 ||
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
  TSGNN_ROWS_DISPATCH(posttrain_head_bwd_kernel, R, (unsigned)((P + 31) / 32), 256, 0);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

int tsgnn_posttrain_rowloss_supported(int C, int R) { return (C >= 2 && C <= PT_ROW_MAXC && R >= 1 && R <= ROWS_MAXR) ? 1 : 0; }

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
