// Hard and semi-hard negative mining on a loaded triplet schedule (the reference's TripletSampler.sampler(embed, hardness):
// Code/sage+gat+diffpool/triplet_sampler.py:51-77, one np.linalg.norm call per (anchor, candidate) pair on the host).  ONE launch
// rewrites column 2 of the [T, 3] schedule the stream kernels gather from; no [T, members] distance matrix in memory.
//
// Numerics as in knn.hip, and for its reason: squared distances are sums of (a_d - x_d)^2 (the product form cancels in fp32 on encoder
// embeddings), so the work is a fraction of a GFLOP on the vector ALU.  Every distance of an entry (candidates, the drawn negative,
// the positive) goes through ONE function with ONE summation order, so equal rows give equal bits and a comparison never sees two
// roundings of the same pair.
//
// Workgroup = 4 waves = 4 schedule entries, the four anchor rows in LDS (16 KB; the value a lane needs is a broadcast).  Lane l of
// wave w walks the candidates at list positions l, l + 64, ... of entry w's negative class and reads ITS candidate row from memory
// with 16-byte loads (the table of a DD-sized dataset is ~300 KB: L2), columns at or past dim read as zero.
//   hardest    a candidate counts only if it is STRICTLY closer than the drawn negative (so the drawn negative wins a tie for the
//              minimum, and a NaN distance never wins); a lane keeps its best under '<' over ascending positions, the wave takes the
//              minimum over (distance bits, list position) — distances are non-negative, so their bits order as integers, and the
//              position sends a tie to the earliest place in the list.
//   semi-hard  the first list position with d(a, j) < d(a, pos): after every stride of 64 positions a ballot of the qualifying lanes
//              ends the walk, the lowest set bit is the answer.
// One writer per entry (lane 0 of its wave, a plain store, only when the negative changes); the only atomic is the optional count.
#include "common.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int MINE_TE = 4;                 // schedule entries (= waves) per workgroup
constexpr int MINE_MAXD = 1024;

// columns at or past `dim` read as zero (rows are 16-byte padded; what the padding holds is the caller's business)
__device__ __forceinline__ float4 mine_load4(const float* row, int c4, int dim) {
  float4 v = reinterpret_cast<const float4*>(row)[c4];
  const int d = 4 * c4;
  if (d + 1 >= dim) v.y = 0.f;
  if (d + 2 >= dim) v.z = 0.f;
  if (d + 3 >= dim) v.w = 0.f;
  return v;
}

// squared distance of the anchor row in LDS and a row in memory: the one summation order of this file
__device__ __forceinline__ float mine_dist2(const float4* __restrict__ a, const float* __restrict__ row, int D4, int dim) {
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
  for (int c = 0; c < D4; ++c) {
    const float4 t = mine_load4(row, c, dim), v = a[c];
    const float dx = v.x - t.x, dy = v.y - t.y, dz = v.z - t.z, dw = v.w - t.w;
    acc.x = fmaf(dx, dx, acc.x); acc.y = fmaf(dy, dy, acc.y); acc.z = fmaf(dz, dz, acc.z); acc.w = fmaf(dw, dw, acc.w);
  }
  return (acc.x + acc.y) + (acc.z + acc.w);
}

__device__ __forceinline__ unsigned long long mine_wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

__device__ __forceinline__ int mine_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <int MODE>
__global__ __launch_bounds__(256) void mine_negatives_kernel(const float* __restrict__ emb, int64_t ld, int n_graphs, int dim,
                                                             const int* __restrict__ class_of, const int* __restrict__ class_ptr,
                                                             const int* __restrict__ members, int n_classes, int* __restrict__ sched,
                                                             int64_t T, int* __restrict__ n_changed) {
  __shared__ float4 as[MINE_TE][MINE_MAXD / 4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int D4 = (dim + 3) >> 2;
  for (int i = threadIdx.x; i < MINE_TE * D4; i += 256) {
    const int w = i / D4, c = i - w * D4;
    const int64_t tt = min((int64_t)blockIdx.x * MINE_TE + w, T - 1);           // (a wave past the last entry loads a copy of it)
    const int a = mine_clamp(sched[3 * tt], 0, n_graphs - 1);
    as[w][c] = mine_load4(emb + (int64_t)a * ld, c, dim);
  }
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * MINE_TE + wid;
  if (t >= T) return;                                                            // (wave-uniform, after the only barrier)

  // indices are clamped into their tables before use, as the gather kernels clamp theirs
  const int neg = mine_clamp(sched[3 * t + 2], 0, n_graphs - 1);
  const int total = max(class_ptr[n_classes], 0);
  const int cls = mine_clamp(class_of[neg], 0, n_classes - 1);
  const int lo = mine_clamp(class_ptr[cls], 0, total), hi = mine_clamp(class_ptr[cls + 1], lo, total);
  const int n = hi - lo;
  const float4* a = as[wid];
  int choice = neg;

  if (MODE == 2) {
    const float d0 = mine_dist2(a, emb + (int64_t)neg * ld, D4, dim);
    float bd = 0.f;
    int bp = -1;
    for (int p = lane; p < n; p += 64) {
      const int j = mine_clamp(members[lo + p], 0, n_graphs - 1);
      const float d = mine_dist2(a, emb + (int64_t)j * ld, D4, dim);
      if (d < d0 && (bp < 0 || d < bd)) { bd = d; bp = p; }
    }
    const unsigned long long key = bp >= 0 ? ((unsigned long long)__float_as_uint(bd) << 32) | (unsigned)bp : ~0ull;
    const unsigned long long m = mine_wave_min_u64(key);
    if (m != ~0ull) choice = mine_clamp(members[lo + (int)(unsigned)(m & 0xffffffffull)], 0, n_graphs - 1);
  } else {
    const int pos = mine_clamp(sched[3 * t + 1], 0, n_graphs - 1);
    const float dp = mine_dist2(a, emb + (int64_t)pos * ld, D4, dim);
    for (int p0 = 0; p0 < n; p0 += 64) {                                         // (p0, n: wave-uniform)
      const int p = p0 + lane;
      bool hit = false;
      if (p < n) {
        const int j = mine_clamp(members[lo + p], 0, n_graphs - 1);
        hit = mine_dist2(a, emb + (int64_t)j * ld, D4, dim) < dp;
      }
      const unsigned long long mask = __ballot(hit);
      if (mask) {
        choice = mine_clamp(members[lo + p0 + (__ffsll((long long)mask) - 1)], 0, n_graphs - 1);
        break;
      }
    }
  }
  if (lane == 0 && choice != sched[3 * t + 2]) {
    sched[3 * t + 2] = choice;
    if (n_changed) atomicAdd(n_changed, 1);
  }
}

}  // namespace

extern "C" {

int tsgnn_mine_supported(int64_t dim, int n_classes) { return dim >= 1 && dim <= MINE_MAXD && n_classes >= 2; }

int tsgnn_mine_negatives_f32(const float* emb, int64_t ld, int64_t n_graphs, int64_t dim, const int32_t* class_of,
                             const int32_t* class_ptr, const int32_t* members, int n_classes, int32_t* sched, int64_t T, int mode,
                             int32_t* n_changed, hipStream_t stream) {
  if (!emb || !class_of || !class_ptr || !members || !sched || T < 1 || n_graphs < 1 || dim < 1 || n_classes < 2 ||
      (mode != 1 && mode != 2) || ld < dim)
    return TSGNN_EINVAL;
  if (!tsgnn_mine_supported(dim, n_classes) || (ld % 4) ||
      (reinterpret_cast<uintptr_t>(emb) & 15) || n_graphs >= 0x7fffffff ||
      T > 0x7fffffff / 3 || n_classes >= 0x7fffffff)
    return TSGNN_EUNSUPPORTED;
  const unsigned grid = (unsigned)((T + MINE_TE - 1) / MINE_TE);
  TSGNN_KNAME("mine_negatives_kernel<%d>", mode);
  if (mode == 1)
    mine_negatives_kernel<1><<<grid, 256, 0, stream>>>(emb, ld, (int)n_graphs, (int)dim, class_of, class_ptr, members, n_classes, sched, T,
                                                       n_changed);
  else
    mine_negatives_kernel<2><<<grid, 256, 0, stream>>>(emb, ld, (int)n_graphs, (int)dim, class_of, class_ptr, members, n_classes, sched, T,
                                                       n_changed);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
