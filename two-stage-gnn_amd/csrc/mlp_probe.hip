// Stage two of the two-stage scheme, the MLP probe: the reference's evaluate_mlp() (Code/sage+gat+diffpool/train_triplet.py:105-183,
// Code/eigengcn/train_triplet.py:138-268) trains Linear(E, h1)-LeakyReLU-Linear(h1, h2)-LeakyReLU-Linear(h2, C) with ONE Adam step per
// training embedding, in row order, and then predicts the validation rows one at a time.  The training loop is a latency chain of n
// dependent rank-1 updates on at most 1024 x 64 weights: a launch per op spends its time between kernels.  Here the whole loop is ONE
// launch of ONE workgroup of 1,024 threads that keeps the network and both Adam moments on the chip from the first sample to the last.
//
// Ownership (the same for all three layers): thread t serves row r = t / 16 of a layer's [out, in] weight with its 16-lane DPP row,
// lane l = t % 16 holding the float4 column chunks l, l + 16, ... of that row.  The forward dot product of row r is the lanes' partial
// sums combined by one DPP row reduction, the rank-1 gradient dz[r] * in[c] and the Adam update touch only the lane's own chunks: the
// W1 slice and its moments stay in registers (3 * NC4 float4, 96 values at dim 512), layers 2 and 3 (one float4 each of weight and
// moments per thread) and the biases in LDS.  Past 512 columns the W1 moments no longer fit the 128-register budget of 16 waves; there
// the kernel keeps W1 in registers and streams each thread's own moment chunks through the caller's moment buffers (L2 resident, never
// shared between threads, so no ordering is needed).  The transposed products of the backward pass (da = W^T dz) go through LDS: every
// thread writes dz[r] * w[r][c] for its four columns, row c's lanes sum the 64 contributions in a fixed order.  Five workgroup barriers
// per sample; sample i + 1's row is requested from memory before sample i's forward pass (one float per thread) and lands in the other
// half of a double buffer.  A wave whose four rows lie past a layer's width skips that layer's arithmetic: an instruction that all 16
// waves execute costs the CU 16 issue slots.  Every reduction has a fixed order, so two runs are bit-identical.  The bias corrections
// 1 - beta^t come from running products kept in double by one lane and handed to the others through LDS one step ahead.  No variant
// uses scratch (-Rpass-analysis=kernel-resource-usage); what that took at NC4 = 8 is said where it was done.
#include "common.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int MP_MAXD = 1024, MP_MAXH = 64, MP_MAXC = 64;
constexpr int MP_T = 1024;                 // threads of the fit workgroup: 64 rows x 16 lanes
constexpr int MP_PS = 65;                  // row stride of the transposed-product staging (floats): column sums read conflict-free
constexpr int MP_REG_D = 512;              // widest input whose W1 moments stay in registers

struct MlpProbeFit {
  const float* x;
  int64_t ld_x;
  const int* cls;
  int64_t n;
  int dim, h1, h2, C;
  float *w1, *b1, *w2, *b2, *w3, *b3;
  float *exp_avg, *exp_avg_sq;             // both or neither: [W1 | b1 | W2 | b2 | W3 | b3]
  double pow1, pow2;                       // beta1^step0, beta2^step0
  double lr, beta1, beta2;
  float eps, slope;
  float* loss;
};

struct AdamStep {
  float omb1, b2, omb2, step, rbc2, eps;   // 1 - beta1, beta2, 1 - beta2, lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t), eps
};

// torch.optim.Adam's update of one value: lerp of the first moment, the second moment, the step on the bias-corrected ratio.
// The square root and the reciprocal are the hardware's 1-ulp instructions: the correctly rounded expansions cost ten instructions and
// half a dozen temporaries each, per value, in a loop whose state already fills the register file.  The denominator is at least eps,
// so the reciprocal never sees a denormal; a second moment below 2^-126 may read as zero next to eps.  g == 0 with zero moments
// leaves p untouched (0 * (1 / eps) == 0).
__device__ __forceinline__ void adam1(float& p, float& m, float& v, float g, const AdamStep& k) {
  m = fmaf(k.omb1, g - m, m);
  v = fmaf(k.omb2 * g, g, v * k.b2);
  p = fmaf(-k.step * m, __builtin_amdgcn_rcpf(fmaf(__builtin_amdgcn_sqrtf(v), k.rbc2, k.eps)), p);
}
// one value after the other: `tie` makes each update wait for the one before it, so the four are not merged into packed
// instructions, whose uniform operands (the six numbers of AdamStep) would each need a register pair of their own
__device__ __forceinline__ void adam1_tied(float& p, float& m, float& v, float g, const AdamStep& k, float& tie) {
  asm volatile("" : "+v"(g) : "v"(tie));
  adam1(p, m, v, g, k);
  tie = p;
}
// TIGHT: the variants whose W1 state fills the register file; the others leave the four updates to the scheduler (measured at E = 64:
// 2.86 us per step against 3.41 with the tight forms everywhere, profiles/r08/mlp_probe_forms.txt)
template <bool TIGHT>
__device__ __forceinline__ void adam4(float4& p, float4& m, float4& v, float s, float4 in, const AdamStep& k) {
  if (TIGHT) {
    float tie = s;
    adam1_tied(p.x, m.x, v.x, s * in.x, k, tie);
    adam1_tied(p.y, m.y, v.y, s * in.y, k, tie);
    adam1_tied(p.z, m.z, v.z, s * in.z, k, tie);
    adam1_tied(p.w, m.w, v.w, s * in.w, k, tie);
  } else {
    adam1(p.x, m.x, v.x, s * in.x, k);
    adam1(p.y, m.y, v.y, s * in.y, k);
    adam1(p.z, m.z, v.z, s * in.z, k);
    adam1(p.w, m.w, v.w, s * in.w, k);
  }
}

// layers 2 and 3, whose state lives in LDS: the thread's four columns first contribute dz[r] * w[r][c] to the transposed product,
// then take their Adam step; TIGHT: one column at a time (the W1 slice leaves a lane few registers)
template <bool TIGHT>
__device__ __forceinline__ void backward_lds(float4* w4, float4* m4, float4* v4, float dz, const float4* in4, float* part, const AdamStep& k) {
  if (!TIGHT) {
    float4 w = *w4, m = *m4, v = *v4;
    part[0] = dz * w.x; part[MP_PS] = dz * w.y; part[2 * MP_PS] = dz * w.z; part[3 * MP_PS] = dz * w.w;
    adam4<false>(w, m, v, dz, *in4, k);
    *w4 = w; *m4 = m; *v4 = v;
    return;
  }
  float* const w = reinterpret_cast<float*>(w4);
  float* const m = reinterpret_cast<float*>(m4);
  float* const v = reinterpret_cast<float*>(v4);
  const float* const in = reinterpret_cast<const float*>(in4);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    asm volatile("" ::: "memory");
    float pw = w[j], pm = m[j], pv = v[j];
    part[j * MP_PS] = dz * pw;
    adam1(pw, pm, pv, dz * in[j], k);
    w[j] = pw; m[j] = pm; v[j] = pv;
  }
}

// columns [c, c + 4) of a row of `lim` values; a null row or a column at or past lim reads as zero and is never written
__device__ __forceinline__ float4 ld4m(const float* row, int c, int lim) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (row) {
    if (c < lim) v.x = row[c];
    if (c + 1 < lim) v.y = row[c + 1];
    if (c + 2 < lim) v.z = row[c + 2];
    if (c + 3 < lim) v.w = row[c + 3];
  }
  return v;
}
__device__ __forceinline__ void st4m(float* row, int c, int lim, float4 v) {
  if (row) {
    if (c < lim) row[c] = v.x;
    if (c + 1 < lim) row[c + 1] = v.y;
    if (c + 2 < lim) row[c + 2] = v.z;
    if (c + 3 < lim) row[c + 3] = v.w;
  }
}
// chunk c4 of a 16-byte aligned, padded row; what lies at or past `dim` (the padding may hold anything) reads as zero
__device__ __forceinline__ float4 ld_row4(const float* row, int c4, int dim) {
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  const int d = 4 * c4;
  if (d < dim) {
    v = reinterpret_cast<const float4*>(row)[c4];
    if (d + 1 >= dim) v.y = 0.f;
    if (d + 2 >= dim) v.z = 0.f;
    if (d + 3 >= dim) v.w = 0.f;
  }
  return v;
}
__device__ __forceinline__ float dot4(float4 a, float4 b, float acc) {
  acc = fmaf(a.x, b.x, acc);
  acc = fmaf(a.y, b.y, acc);
  acc = fmaf(a.z, b.z, acc);
  return fmaf(a.w, b.w, acc);
}
// the same value behind a fence for the optimiser: what is derived from it afterwards is computed afresh there instead of being kept
// in registers from an earlier use (the column masks of the prologue would otherwise stay live through the whole sample loop)
__device__ __forceinline__ int refreshed(int v) {
  asm volatile("" : "+v"(v));
  return v;
}
__device__ __forceinline__ int refreshed_uniform(int v) {                      // the same for a value all lanes share
  asm volatile("" : "+s"(v));
  return v;
}
__device__ __forceinline__ float leaky(float v, float slope) { return v > 0.f ? v : slope * v; }
__device__ __forceinline__ float leaky_grad(float v, float slope) { return v > 0.f ? 1.f : slope; }   // at exactly 0: slope (torch)

__device__ __forceinline__ void bias_corrections(double p1, double p2, double lr, float* out) {
  out[0] = (float)(lr / (1.0 - p1));
  out[1] = (float)(1.0 / sqrt(1.0 - p2));
}

// NC4: float4 chunks of a W1 row per lane (dim <= 64 * NC4).  STREAM: the W1 moments live in exp_avg / exp_avg_sq, not in registers.
template <int NC4, bool STREAM>
__global__ __launch_bounds__(MP_T) void mlp_probe_fit_kernel(const MlpProbeFit a) {
  __shared__ float4 st23[6][MP_T];                     // layer 2: weight, m, v; layer 3: weight, m, v (one float4 per thread each)
  __shared__ float4 xs[2][MP_MAXD / 4];                // the current sample's row and the next one's
  __shared__ float part3[MP_MAXH * MP_PS], part2[MP_MAXH * MP_PS];   // [input column][output row] of dz[r] * w[r][c]
  __shared__ float bs[3][3][MP_MAXH];                  // b1, b2, b3 with their moments: row r's belong to lane 0 of row r
  __shared__ float zs[2][2][MP_MAXH];                  // pre-activations of layers 1 and 2 of step i in zs[i & 1]
  __shared__ float4 act1[MP_MAXH / 4], act2[MP_MAXH / 4];
  __shared__ float logit[MP_MAXC];
  __shared__ float hyp[2][2];                          // (lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)) of step i in hyp[i & 1]
  __shared__ double pw[2];                             // beta1^t, beta2^t: the running products, one lane's business

  int tid = threadIdx.x, r = tid >> 4, l = tid & 15;
  const int dim = a.dim, h1 = a.h1, h2 = a.h2, C = a.C;
  const float slope = a.slope;
  const int64_t o_b1 = (int64_t)h1 * dim, o_w2 = o_b1 + h1, o_b2 = o_w2 + (int64_t)h2 * h1, o_w3 = o_b2 + h2, o_b3 = o_w3 + (int64_t)C * h2;
  float* const ea = a.exp_avg;
  float* const es = a.exp_avg_sq;
  AdamStep K;
  K.omb1 = (float)(1.0 - a.beta1);
  K.b2 = (float)a.beta2;
  K.omb2 = (float)(1.0 - a.beta2);
  K.eps = a.eps;

  // ---- the network and its moments come on chip: layers 2 and 3 first, while the registers of the W1 slice are still free
  st23[0][tid] = ld4m(r < h2 ? a.w2 + (int64_t)r * h1 : nullptr, 4 * l, h1);
  st23[1][tid] = ld4m((r < h2 && ea) ? ea + o_w2 + (int64_t)r * h1 : nullptr, 4 * l, h1);
  st23[2][tid] = ld4m((r < h2 && es) ? es + o_w2 + (int64_t)r * h1 : nullptr, 4 * l, h1);
  st23[3][tid] = ld4m(r < C ? a.w3 + (int64_t)r * h2 : nullptr, 4 * l, h2);
  st23[4][tid] = ld4m((r < C && ea) ? ea + o_w3 + (int64_t)r * h2 : nullptr, 4 * l, h2);
  st23[5][tid] = ld4m((r < C && es) ? es + o_w3 + (int64_t)r * h2 : nullptr, 4 * l, h2);
  if (l == 0) {                                                                 // (row r's bias state: lane 0 of the row, from here to the end)
    bs[0][0][r] = r < h1 ? a.b1[r] : 0.f;
    bs[0][1][r] = (r < h1 && ea) ? ea[o_b1 + r] : 0.f;
    bs[0][2][r] = (r < h1 && es) ? es[o_b1 + r] : 0.f;
    bs[1][0][r] = r < h2 ? a.b2[r] : 0.f;
    bs[1][1][r] = (r < h2 && ea) ? ea[o_b2 + r] : 0.f;
    bs[1][2][r] = (r < h2 && es) ? es[o_b2 + r] : 0.f;
    bs[2][0][r] = r < C ? a.b3[r] : 0.f;
    bs[2][1][r] = (r < C && ea) ? ea[o_b3 + r] : 0.f;
    bs[2][2][r] = (r < C && es) ? es[o_b3 + r] : 0.f;
  }
  __builtin_amdgcn_sched_barrier(0);
  float4 w1[NC4], m1[STREAM ? 1 : NC4], v1[STREAM ? 1 : NC4];
  {
    const float* const w1row = r < h1 ? a.w1 + (int64_t)r * dim : nullptr;
    const float* const m1row = (r < h1 && ea) ? ea + (int64_t)r * dim : nullptr;
    const float* const v1row = (r < h1 && es) ? es + (int64_t)r * dim : nullptr;
#pragma unroll
    for (int k = 0; k < NC4; ++k) {
      const int c = 4 * (l + 16 * k);
      w1[k] = ld4m(w1row, c, dim);
      if (!STREAM) {
        m1[STREAM ? 0 : k] = ld4m(m1row, c, dim);
        v1[STREAM ? 0 : k] = ld4m(v1row, c, dim);
      }
      if (NC4 >= 8) __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (tid < MP_MAXD / 4) xs[0][tid] = ld_row4(a.x, tid, dim);
  // A wave serves four rows of every layer; where all four lie past the layer's width (Linear(32, 2): rows 2 .. 63) the wave skips
  // the layer's arithmetic, forward and backward, and only keeps the barriers.  What it would have written is zero, once:
  for (int j = tid; j < MP_MAXH * MP_PS; j += MP_T) part3[j] = part2[j] = 0.f;
  if (tid < MP_MAXH) {
    reinterpret_cast<float*>(act1)[tid] = reinterpret_cast<float*>(act2)[tid] = 0.f;
    zs[0][0][tid] = zs[0][1][tid] = zs[1][0][tid] = zs[1][1][tid] = 0.f;
  }
  constexpr bool TIGHT = NC4 >= 8;
  const int row0 = __builtin_amdgcn_readfirstlane(tid >> 4);
  const bool on1 = row0 < h1, on2 = row0 < h2, on3 = row0 < C;
  if (tid == MP_T - 16) {                                                       // beta^t of the first step, t = step0 + 1
    pw[0] = a.pow1 * a.beta1;
    pw[1] = a.pow2 * a.beta2;
    bias_corrections(pw[0], pw[1], a.lr, hyp[0]);
  }
  __syncthreads();

  for (int64_t i = 0; i < a.n; ++i) {
    const int cur = (int)(i & 1);
    tid = refreshed(tid); r = tid >> 4; l = tid & 15;                           // (addresses are formed where they are used, not kept)
    // sample i + 1's row: one value per thread, requested before the forward pass, stored to LDS behind the third layer; what lies
    // at or past dim (the padding may hold anything) reads as zero
    const int dim_i = refreshed_uniform(dim);
    const float xn = (tid < dim_i && i + 1 < a.n) ? a.x[(i + 1) * a.ld_x + tid] : 0.f;

    // ---- forward
    if (on1) {
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < NC4; ++k) {
        if (64 * k < dim_i) acc = dot4(w1[k], xs[cur][l + 16 * k], acc);        // (chunks past the row hold zeros)
        if (TIGHT) __builtin_amdgcn_sched_barrier(0);                           // one chunk of x at a time: the state fills the register file
      }
      acc = row16_sum(acc);
      if (l == 0) {
        const float z = acc + bs[0][0][r];
        zs[cur][0][r] = z;
        reinterpret_cast<float*>(act1)[r] = leaky(z, slope);
      }
    }
    __syncthreads();                                                            // A
    tid = refreshed(tid); r = tid >> 4; l = tid & 15;
    if (on2) {
      const float acc = row16_sum(dot4(st23[0][tid], act1[l], 0.f));
      if (l == 0) {
        const float z = acc + bs[1][0][r];
        zs[cur][1][r] = z;
        reinterpret_cast<float*>(act2)[r] = leaky(z, slope);
      }
    }
    __syncthreads();                                                            // B
    tid = refreshed(tid); r = tid >> 4; l = tid & 15;
    if (on3) {
      const float acc = row16_sum(dot4(st23[3][tid], act2[l], 0.f));
      if (l == 0) logit[r] = acc + bs[2][0][r];
    }
    __syncthreads();                                                            // C
    tid = refreshed(tid); r = tid >> 4; l = tid & 15;

    // ---- cross-entropy in log-sum-exp form
    K.step = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, hyp[cur][0])));
    K.rbc2 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, hyp[cur][1])));
    if (on3) {
      const int y = min(max(a.cls[i], 0), C - 1);
      // softmax - onehot without cancellation: the true class gets -(sum of the others' probabilities), not p - 1 (a well
      // classified row has p within an ulp of 1, and Adam's normalisation turns the relative error of a tiny gradient into a
      // full-sized step)
      float mx = logit[0];
#pragma clang loop vectorize(disable) unroll(disable)
      for (int c = 1; c < C; ++c) mx = fmaxf(mx, logit[c]);
      float so = 0.f;
#pragma clang loop vectorize(disable) unroll(disable)
      for (int c = 0; c < C; ++c) so += c == y ? 0.f : expf(logit[c] - mx);      // (in class order: a fixed sum)
      const float zy = logit[y], se = expf(zy - mx) + so, inv = 1.f / se;
      if (tid == 0 && a.loss) a.loss[i] = (mx - zy) + logf(se);
      const float dz3 = r < C ? (r == y ? -so : expf(logit[r < C ? r : 0] - mx)) * inv : 0.f;
      backward_lds<TIGHT>(&st23[3][tid], &st23[4][tid], &st23[5][tid], dz3, &act2[l], part3 + 4 * l * MP_PS + r, K);
      if (l == 0) adam1(bs[2][0][r], bs[2][1][r], bs[2][2][r], dz3, K);
    }
    reinterpret_cast<float*>(xs[cur ^ 1])[tid] = xn;
    __syncthreads();                                                            // D
    tid = refreshed(tid); r = tid >> 4; l = tid & 15;

    // ---- layer 2 backward
    if (on2) {
      const float* const q = part3 + r * MP_PS + l;
      const float dz2 = row16_sum((q[0] + q[16]) + (q[32] + q[48])) * leaky_grad(zs[cur][1][r], slope);
      backward_lds<TIGHT>(&st23[0][tid], &st23[1][tid], &st23[2][tid], dz2, &act1[l], part2 + 4 * l * MP_PS + r, K);
      if (l == 0) adam1(bs[1][0][r], bs[1][1][r], bs[1][2][r], dz2, K);
    }
    __syncthreads();                                                            // E
    tid = refreshed(tid); r = tid >> 4; l = tid & 15;

    // ---- layer 1 backward: the rank-1 gradient dz1[r] * x on the lane's own chunks
    if (on1) {
      const float* const q = part2 + r * MP_PS + l;
      const float dz1 = row16_sum((q[0] + q[16]) + (q[32] + q[48])) * leaky_grad(zs[cur][0][r], slope);
#pragma unroll
      for (int k = 0; k < NC4; ++k) {
        if (64 * k >= dim_i) continue;                                          // (a chunk past the row: zero gradient, nothing moves)
        const float4 xv = xs[cur][l + 16 * k];
        if (STREAM) {
          const int c = 4 * (l + 16 * k);
          float* const m1row = r < h1 ? ea + (int64_t)r * dim_i : nullptr;     // (this variant is launched with moment buffers only)
          float* const v1row = r < h1 ? es + (int64_t)r * dim_i : nullptr;
          float4 m = ld4m(m1row, c, dim_i), v = ld4m(v1row, c, dim_i);
          adam4<TIGHT>(w1[k], m, v, dz1, xv, K);
          st4m(m1row, c, dim_i, m);
          st4m(v1row, c, dim_i, v);
        } else {
          adam4<TIGHT>(w1[k], m1[STREAM ? 0 : k], v1[STREAM ? 0 : k], dz1, xv, K);
        }
        __builtin_amdgcn_sched_barrier(0);                                      // one chunk at a time: the state fills the register file
      }
      if (l == 0) adam1(bs[0][0][r], bs[0][1][r], bs[0][2][r], dz1, K);
    }
    if (tid == MP_T - 16) {                                                     // next step's bias corrections, one step ahead
      pw[0] *= a.beta1;
      pw[1] *= a.beta2;
      bias_corrections(pw[0], pw[1], a.lr, hyp[cur ^ 1]);
    }
  }

  // ---- the trained network and the moments go back
  {
    const int dim_e = refreshed_uniform(dim);
    float* const w1row = r < h1 ? a.w1 + (int64_t)r * dim_e : nullptr;
    float* const m1row = (r < h1 && ea) ? ea + (int64_t)r * dim_e : nullptr;
    float* const v1row = (r < h1 && es) ? es + (int64_t)r * dim_e : nullptr;
#pragma unroll
    for (int k = 0; k < NC4; ++k) {
      const int c = 4 * (l + 16 * k);
      st4m(w1row, c, dim_e, w1[k]);
      if (!STREAM) {
        st4m(m1row, c, dim_e, m1[STREAM ? 0 : k]);
        st4m(v1row, c, dim_e, v1[STREAM ? 0 : k]);
      }
      if (NC4 >= 8) __builtin_amdgcn_sched_barrier(0);
    }
  }
  st4m(r < h2 ? a.w2 + (int64_t)r * h1 : nullptr, 4 * l, h1, st23[0][tid]);
  st4m(r < C ? a.w3 + (int64_t)r * h2 : nullptr, 4 * l, h2, st23[3][tid]);
  if (ea) {
    st4m(r < h2 ? ea + o_w2 + (int64_t)r * h1 : nullptr, 4 * l, h1, st23[1][tid]);
    st4m(r < h2 ? es + o_w2 + (int64_t)r * h1 : nullptr, 4 * l, h1, st23[2][tid]);
    st4m(r < C ? ea + o_w3 + (int64_t)r * h2 : nullptr, 4 * l, h2, st23[4][tid]);
    st4m(r < C ? es + o_w3 + (int64_t)r * h2 : nullptr, 4 * l, h2, st23[5][tid]);
  }
  if (l == 0) {
    if (r < h1) a.b1[r] = bs[0][0][r];
    if (r < h2) a.b2[r] = bs[1][0][r];
    if (r < C) a.b3[r] = bs[2][0][r];
    if (ea) {
      if (r < h1) { ea[o_b1 + r] = bs[0][1][r]; es[o_b1 + r] = bs[0][2][r]; }
      if (r < h2) { ea[o_b2 + r] = bs[1][1][r]; es[o_b2 + r] = bs[1][2][r]; }
      if (r < C) { ea[o_b3 + r] = bs[2][1][r]; es[o_b3 + r] = bs[2][2][r]; }
    }
  }
}

// ------------------------------------------------------------------------------------------------ predict
// One wave per query row, four rows per workgroup.  Lane j is unit j of each layer in turn and walks its own weight row (the rows of
// a wave's 64 lanes stay in L1 across the walk); the row of inputs is an LDS broadcast.  Four partial sums per lane, combined in a
// fixed order.  The argmax over the logits is a wave maximum of (ordered logit bits, 63 - class): a tie goes to the lowest class.
constexpr int MP_PQ = 4;

__device__ __forceinline__ float lane_dot(const float* __restrict__ w, const float* in, int K) {
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  int k = 0;
  for (; k + 4 <= K; k += 4) {
    s0 = fmaf(w[k], in[k], s0);
    s1 = fmaf(w[k + 1], in[k + 1], s1);
    s2 = fmaf(w[k + 2], in[k + 2], s2);
    s3 = fmaf(w[k + 3], in[k + 3], s3);
  }
  if (k < K) s0 = fmaf(w[k], in[k], s0);
  if (k + 1 < K) s1 = fmaf(w[k + 1], in[k + 1], s1);
  if (k + 2 < K) s2 = fmaf(w[k + 2], in[k + 2], s2);
  return (s0 + s1) + (s2 + s3);
}

__global__ __launch_bounds__(64 * MP_PQ) void mlp_probe_predict_kernel(const float* __restrict__ q, int64_t ld_q, int64_t n_query, int dim,
                                                                       int h1, int h2, int C, const float* __restrict__ w1,
                                                                       const float* __restrict__ b1, const float* __restrict__ w2,
                                                                       const float* __restrict__ b2, const float* __restrict__ w3,
                                                                       const float* __restrict__ b3, float slope, float* __restrict__ logits,
                                                                       int* __restrict__ pred, const int* __restrict__ query_class,
                                                                       int* __restrict__ correct) {
  __shared__ float4 qs[MP_PQ][MP_MAXD / 4];
  __shared__ float hs[MP_PQ][2][MP_MAXH];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * MP_PQ + wid;
  const int64_t src = min(row, n_query - 1);                                   // (a wave past the last query works on a copy of it)
  const int D4 = (dim + 3) >> 2;
  for (int c = lane; c < D4; c += 64) qs[wid][c] = ld_row4(q + src * ld_q, c, dim);
  __syncthreads();
  const float* in = reinterpret_cast<const float*>(qs[wid]);
  hs[wid][0][lane] = lane < h1 ? leaky(lane_dot(w1 + (int64_t)lane * dim, in, dim) + b1[lane], slope) : 0.f;
  __syncthreads();
  hs[wid][1][lane] = lane < h2 ? leaky(lane_dot(w2 + (int64_t)lane * h1, hs[wid][0], h1) + b2[lane], slope) : 0.f;
  __syncthreads();
  const float z = lane < C ? lane_dot(w3 + (int64_t)lane * h2, hs[wid][1], h2) + b3[lane] : 0.f;
  unsigned long long key = lane < C ? ((unsigned long long)f32_ordered(z) << 32) | (unsigned)(63 - lane) : 0ull;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off, 64);
    key = o > key ? o : key;
  }
  const int p = 63 - (int)(key & 63ull);
  if (row < n_query) {
    if (logits && lane < C) logits[row * C + lane] = z;
    if (lane == 0) {
      pred[row] = p;
      if (query_class && correct && query_class[row] == p) atomicAdd(correct, 1);
    }
  }
}

bool mlp_probe_dims_ok(int64_t dim, int h1, int h2, int C) {
  return dim >= 1 && dim <= MP_MAXD && h1 >= 1 && h1 <= MP_MAXH && h2 >= 1 && h2 <= MP_MAXH && C >= 2 && C <= MP_MAXC;
}

}  // namespace

extern "C" {

int tsgnn_mlp_probe_supported(int64_t dim, int h1, int h2, int n_classes) { return mlp_probe_dims_ok(dim, h1, h2, n_classes) ? 1 : 0; }

int tsgnn_mlp_probe_fit_f32(const float* x, int64_t ld_x, const int* cls, int64_t n, int64_t dim, int h1, int h2, int n_classes, float* w1,
                            float* b1, float* w2, float* b2, float* w3, float* b3, float* exp_avg, float* exp_avg_sq, int64_t step0,
                            double lr, double beta1, double beta2, double eps, double negative_slope, float* loss, hipStream_t stream) {
  if (!x || !cls || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || n < 1 || step0 < 0 || !mlp_probe_dims_ok(dim, h1, h2, n_classes) ||
      ld_x < dim || (ld_x % 4) || (exp_avg == nullptr) != (exp_avg_sq == nullptr) || !(beta1 >= 0.0 && beta1 < 1.0) ||
      !(beta2 >= 0.0 && beta2 < 1.0))
    return TSGNN_EINVAL;
  if ((reinterpret_cast<uintptr_t>(x) & 15) || (dim > MP_REG_D && !exp_avg))   // (past 512 columns the W1 moments live in the caller's buffers)
    return TSGNN_EUNSUPPORTED;
  MlpProbeFit a;
  a.x = x; a.ld_x = ld_x; a.cls = cls; a.n = n;
  a.dim = (int)dim; a.h1 = h1; a.h2 = h2; a.C = n_classes;
  a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.w3 = w3; a.b3 = b3;
  a.exp_avg = exp_avg; a.exp_avg_sq = exp_avg_sq;
  a.pow1 = pow(beta1, (double)step0); a.pow2 = pow(beta2, (double)step0);
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2;
  a.eps = (float)eps; a.slope = (float)negative_slope;
  a.loss = loss;
#define TSGNN_MLP_FIT(NC4, STREAM)                                                       \
  do {                                                                                   \
    TSGNN_KNAME("mlp_probe_fit_kernel<%d, %d>", NC4, (int)STREAM);                       \
    mlp_probe_fit_kernel<NC4, STREAM><<<1, MP_T, 0, stream>>>(a);                        \
  } while (0)
  if (dim <= 64) TSGNN_MLP_FIT(1, false);
  else if (dim <= 128) TSGNN_MLP_FIT(2, false);
  else if (dim <= 256) TSGNN_MLP_FIT(4, false);
  else if (dim <= MP_REG_D) TSGNN_MLP_FIT(8, false);
  else TSGNN_MLP_FIT(16, true);
#undef TSGNN_MLP_FIT
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

int tsgnn_mlp_probe_predict_f32(const float* q, int64_t ld_q, int64_t n_query, int64_t dim, int h1, int h2, int n_classes, const float* w1,
                                const float* b1, const float* w2, const float* b2, const float* w3, const float* b3,
                                double negative_slope, float* logits, int* pred, const int* query_class, int* correct,
                                hipStream_t stream) {
  if (!q || !pred || !w1 || !b1 || !w2 || !b2 || !w3 || !b3 || n_query < 1 || !mlp_probe_dims_ok(dim, h1, h2, n_classes) || ld_q < dim ||
      (ld_q % 4) || (query_class == nullptr) != (correct == nullptr))
    return TSGNN_EINVAL;
  if ((reinterpret_cast<uintptr_t>(q) & 15) || (n_query + MP_PQ - 1) / MP_PQ > 0x7fffffff) return TSGNN_EUNSUPPORTED;
  TSGNN_KNAME("mlp_probe_predict_kernel");
  mlp_probe_predict_kernel<<<(unsigned)((n_query + MP_PQ - 1) / MP_PQ), 64 * MP_PQ, 0, stream>>>(
      q, ld_q, n_query, (int)dim, h1, h2, n_classes, w1, b1, w2, b2, w3, b3, (float)negative_slope, logits, pred, query_class, correct);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
