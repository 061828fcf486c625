// Stage two of the two-stage scheme: brute-force k-nearest-neighbour classification of embedding rows (the reference's evaluate():
// Code/sage+gat+diffpool/train_triplet.py:78-94, Code/sag/train_triplet.py:60-73 fit sklearn's KNeighborsClassifier(n_neighbors=3) on
// the host).  Distances, selection, vote and the confusion matrix in ONE launch; no [n_query, n_train] matrix in memory.
//
// Numerics first: squared distances are sums of (q_d - x_d)^2.  The product form |q|^2 + |x|^2 - 2 q.x cancels in fp32 on encoder
// embeddings (they share a large common component: map_model's bias, the all-negative log_softmax rows of Net), so there is nothing
// for an fp32 MFMA to do here; the whole problem is a fraction of a GFLOP on the vector ALU and the kernel is shaped by data movement.
//
// Workgroup = 4 waves = 4 queries, whole query rows in LDS.  The training rows stream through LDS in tiles of 64 rows x 128 columns
// (float4, rows padded by one float4: a lane reads ITS row with 16-byte LDS reads and no bank conflict, the query value is a broadcast).
// Lane l of wave w accumulates the distance of (query w, row r0 + l), so a wave sees every training row of its query and no merge
// across waves exists.  Every lane keeps a sorted list of its K best (K = compile-time bound of k, constant indices only: registers,
// no private segment); a lane's rows arrive in ascending index, so a strict '<' keeps equal distances in index order.  The k winners
// are popped off the 64 list heads by a wave minimum over (distance bits, index) — distances are non-negative, so their bit patterns
// order as integers and the index breaks ties towards the lower row.  Lane c counts the votes of class c; the prediction is the
// maximum over (count, 63 - c): ties go to the smallest class index, as sklearn resolves them.  DD-sized evaluation: 1,168 queries =
// 292 workgroups on 256 CUs, three resident per CU (50 KB of LDS each).
#include "common.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int KNN_TQ = 4;                  // queries (= waves) per workgroup
constexpr int KNN_TR = 64;                 // training rows per tile (one per lane)
constexpr int KNN_DC4 = 32;                // float4 columns per tile
constexpr int KNN_MAXD = 1024, KNN_MAXK = 16, KNN_MAXC = 64;
constexpr int KNN_NONE = 0x7fffffff;

// columns at or past `dim` read as zero in both operands (rows are 16-byte padded; what the padding holds is the caller's business)
__device__ __forceinline__ float4 knn_load4(const float* row, int c4, int dim) {
  float4 v = reinterpret_cast<const float4*>(row)[c4];
  const int d = 4 * c4;
  if (d + 1 >= dim) v.y = 0.f;
  if (d + 2 >= dim) v.z = 0.f;
  if (d + 3 >= dim) v.w = 0.f;
  return v;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

template <int K>
__global__ __launch_bounds__(256) void knn_classify_kernel(const float* __restrict__ train, int64_t ld_train,
                                                           const int* __restrict__ train_class, int64_t n_train,
                                                           const float* __restrict__ query, int64_t ld_query, int64_t n_query, int dim, int k,
                                                           int n_classes, const int* __restrict__ query_class, int* __restrict__ confusion,
                                                           int* __restrict__ pred, int* __restrict__ nbr_index, float* __restrict__ nbr_dist) {
  __shared__ float4 qs[KNN_TQ][KNN_MAXD / 4];
  __shared__ float4 ts[KNN_TR][KNN_DC4 + 1];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int D4 = (dim + 3) >> 2;
  const int64_t q = (int64_t)blockIdx.x * KNN_TQ + wid;
  for (int i = threadIdx.x; i < KNN_TQ * D4; i += 256) {
    const int w = i / D4, c = i - w * D4;
    const int64_t qq = min((int64_t)blockIdx.x * KNN_TQ + w, n_query - 1);      // (a wave past the last query works on a copy of it)
    qs[w][c] = knn_load4(query + qq * ld_query, c, dim);
  }
  float bd[K];
  int bi[K];
#pragma unroll
  for (int j = 0; j < K; ++j) { bd[j] = __builtin_inff(); bi[j] = KNN_NONE; }

  for (int64_t r0 = 0; r0 < n_train; r0 += KNN_TR) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int d0 = 0; d0 < D4; d0 += KNN_DC4) {
      const int nc = min(KNN_DC4, D4 - d0);
      const int shc = nc <= 1 ? 0 : 32 - __clz(nc - 1);                          // columns rounded up to a power of two: index by shifts
      __syncthreads();                                                           // the tile's readers are done (first pass: qs is written)
      for (int i = threadIdx.x; i < (KNN_TR << shc); i += 256) {
        const int row = i >> shc, c = i & ((1 << shc) - 1);
        if (c < nc) ts[row][c] = knn_load4(train + min(r0 + row, n_train - 1) * ld_train, d0 + c, dim);
      }
      __syncthreads();
#pragma unroll 4
      for (int c = 0; c < nc; ++c) {
        const float4 t = ts[lane][c], v = qs[wid][d0 + c];
        const float dx = v.x - t.x, dy = v.y - t.y, dz = v.z - t.z, dw = v.w - t.w;
        acc.x = fmaf(dx, dx, acc.x); acc.y = fmaf(dy, dy, acc.y); acc.z = fmaf(dz, dz, acc.z); acc.w = fmaf(dw, dw, acc.w);
      }
    }
    const float d = (acc.x + acc.y) + (acc.z + acc.w);
    if (r0 + lane < n_train && d < bd[K - 1]) {
      bd[K - 1] = d; bi[K - 1] = (int)(r0 + lane);
#pragma unroll
      for (int j = K - 1; j > 0; --j) {
        if (bd[j] < bd[j - 1]) {
          const float td = bd[j]; bd[j] = bd[j - 1]; bd[j - 1] = td;
          const int ti = bi[j]; bi[j] = bi[j - 1]; bi[j - 1] = ti;
        }
      }
    }
  }

  int votes = 0, my_i = -1;
  float my_d = 0.f;
  for (int r = 0; r < k; ++r) {
    const unsigned long long key = ((unsigned long long)__float_as_uint(bd[0]) << 32) | (unsigned)bi[0];
    const unsigned long long m = wave_min_u64(key);
    if (key == m) {                                                              // pop the winner's head (keys of real rows are unique)
#pragma unroll
      for (int j = 0; j + 1 < K; ++j) { bd[j] = bd[j + 1]; bi[j] = bi[j + 1]; }
      bd[K - 1] = __builtin_inff(); bi[K - 1] = KNN_NONE;
    }
    const int wi = (int)(unsigned)(m & 0xffffffffull);
    const bool real = wi != KNN_NONE;                                            // (fewer than k comparable rows: NaN inputs)
    const int cls = real ? train_class[wi] : -1;
    if (lane == cls) ++votes;
    if (lane == r) { my_i = real ? wi : -1; my_d = sqrtf(__uint_as_float((unsigned)(m >> 32))); }
  }
  unsigned best = votes > 0 ? ((unsigned)votes << 8) | (unsigned)(63 - lane) : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, off, 64));
  const int p = best ? 63 - (int)(best & 255u) : 0;
  if (q < n_query) {
    if (lane == 0) {
      pred[q] = p;
      if (query_class && confusion) {
        const int t = query_class[q];
        if (t >= 0 && t < n_classes && p < n_classes) atomicAdd(confusion + (int64_t)t * n_classes + p, 1);
      }
    }
    if (lane < k) {
      if (nbr_index) nbr_index[q * k + lane] = my_i;
      if (nbr_dist) nbr_dist[q * k + lane] = my_d;
    }
  }
}

}  // namespace

extern "C" {

int tsgnn_knn_supported(int64_t dim, int k, int n_classes) {
  return dim >= 1 && dim <= KNN_MAXD && k >= 1 && k <= KNN_MAXK && n_classes >= 1 && n_classes <= KNN_MAXC;
}

int tsgnn_knn_classify_f32(const float* train, int64_t ld_train, const int* train_class, int64_t n_train, const float* query,
                           int64_t ld_query, int64_t n_query, int64_t dim, int k, int n_classes, const int* query_class, int* confusion,
                           int* pred, int* nbr_index, float* nbr_dist, hipStream_t stream) {
  if (!train || !train_class || !query || !pred || n_train < 1 || n_query < 1 || dim < 1 || k < 1 || n_classes < 1 || k > n_train ||
      ld_train < dim || ld_query < dim)
    return TSGNN_EINVAL;
  const int64_t pad = (dim + 3) / 4 * 4;
  if (!tsgnn_knn_supported(dim, k, n_classes) || (ld_train % 4) || (ld_query % 4) || ld_train < pad || ld_query < pad ||
      ((reinterpret_cast<uintptr_t>(train) | reinterpret_cast<uintptr_t>(query)) & 15) || n_train >= KNN_NONE ||
      (n_query + KNN_TQ - 1) / KNN_TQ > 0x7fffffff)
    return TSGNN_EUNSUPPORTED;
  const unsigned grid = (unsigned)((n_query + KNN_TQ - 1) / KNN_TQ);
#define TSGNN_KNN_LAUNCH(K)                                                                                                         \
  do {                                                                                                                              \
    TSGNN_KNAME("knn_classify_kernel<%d>", K);                                                                                      \
    knn_classify_kernel<K><<<grid, 256, 0, stream>>>(train, ld_train, train_class, n_train, query, ld_query, n_query, (int)dim, k, \
                                                     n_classes, query_class, confusion, pred, nbr_index, nbr_dist);                \
  } while (0)
  if (k == 1) TSGNN_KNN_LAUNCH(1);
  else if (k <= 4) TSGNN_KNN_LAUNCH(4);
  else if (k <= 8) TSGNN_KNN_LAUNCH(8);
  else TSGNN_KNN_LAUNCH(16);
#undef TSGNN_KNN_LAUNCH
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
