// DiffPool level-0 contraction (encoders.py:374-375: X' = S^T Z, A' = S^T A S) on a CAPACITY-PADDED batch, the batch the gather
// launch of a stream writes (csrc/triplet_stream.hip, ingest.CapacityBatch).  Its rows are
//     [0, n_tot)                   real rows, n_tot = graph_ptr[B] — read on the DEVICE: the host never knows which graphs a replay holds
//     [n_tot, row_cap)             padding rows of a dummy graph
//     [row_cap, row_cap + nmax)    ghost-slot rows
// and the neighbours of a row come from the neighbour table (ell, width 4 / 8 / 16) and its CSR tail; there are no CSR arrays, no
// host-side sizes and no host-built slab lists (what diffpool._ContractRows reads).
//
// RELIED ON: the arena such a batch is gathered from holds UNIT weights and a SYMMETRIC adjacency (triplet_stream.pack_arena
// rejects every graph that has neither).  So AS[i] is a plain sum of neighbour rows, and in the backward
//     d(AS) = S dA'  =>  dS += A^T d(AS) = A S dA' = (AS) dA'
// so that      dS_b = Z_b dX'_b^T + (AS)_b (dA'_b + dA'_b^T) ,   dZ_b = S_b dX'_b :
// d(AS) is never materialised and the transposed SpMM launch of the CSR route does not exist here.
//
//   tsgnn_ell_rowsum_f32         AS = A S over table + tail; rows >= n_tot are STORED as zeros (a NaN in a padding row of S stays there)
//   forward                      tsgnn_ragged_tn_direct_ro_f32 (ragged.hip) on (S, Z, AS): it reads graph_ptr on the device already
//   tsgnn_contract_cap_bwd_f32   (dX', dA') -> (dZ, dS) in one launch, the max readout's gradient folded into dZ
//
// The backward: a workgroup finds its slab of <= 32 rows of ONE graph by walking graph_ptr (<= 8 graphs, as triplet_gather_kernel
// walks its records); a slab's 32 x 32 output tiles (ceil(K / 32) of dS, depth F + K; ceil(F / 32) of dZ, depth K) are dealt round
// robin, heaviest first, to the 4 * split waves of the slab's `split` workgroups.  Waves share nothing: every operand comes from
// memory (L2) in 16-byte pieces along the contracted index — lane (i, h) of v_mfma_f32_32x32x2_f32 takes k = 8 g + 4 h .. + 3 of
// group g for BOTH operands, so a row-major A row and a row of a TRANSPOSED B operand (dX'^T, dA'^T) are one float4 each; dX'_b
// (154 KB at K = 100, F = 384) would not fit LDS beside dA'_b.  No LDS, no atomics; every output word has one writer (a tile's
// wave, or the zero crew: the workgroups beyond the batch's slabs, which clear rows [n_tot, row_cap + nmax) of dS and dZ — the
// stacks' weight-gradient launches sum over every row); sums run in a fixed order, whatever `split` is.
#include "common.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int CC_MAX_B = 8;
constexpr int CC_KMAX = 128, CC_FMAX = 384;
constexpr int CC_ZERO_BLOCKS = 128;            // workgroups that only clear rows, beside the idle ones of the slab bound
typedef float cc_f32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int cc_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float4 cc_keep(bool ok, const float4& v) { return make_float4(ok ? v.x : 0.f, ok ? v.y : 0.f, ok ? v.z : 0.f, ok ? v.w : 0.f); }

// ---------------------------------------------------------------- AS = A S over the neighbour table and its tail
struct RowSum {
  const int* ell; int W; const int* tail_ptr; const int* tail_col; int64_t tail_cap;
  const int* graph_ptr; int B; int64_t row_cap, rows;
  const float* S; int64_t ldS; int K4; float* out; int64_t ldo;
};

// 32 lanes per row (lane q: columns 4 q .. 4 q + 3), 8 rows per workgroup.  The sum runs over the table's entries in order, then
// over the tail's: one order, whatever the launch.
__global__ __launch_bounds__(256) void ell_rowsum_kernel(RowSum a) {
  const int64_t r = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5);
  const int q = threadIdx.x & 31;
  if (r >= a.rows || q >= a.K4) return;
  const int n_tot = cc_clamp(a.graph_ptr[a.B], 0, (int)a.row_cap);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (r < n_tot) {
    const float* sq = a.S + 4 * q;
    auto add = [&](int j) {                                  // (an id outside the real rows — never written by the gather — is skipped)
      const bool ok = (unsigned)j < (unsigned)n_tot;
      const float4 v = *reinterpret_cast<const float4*>(sq + (int64_t)(ok ? j : 0) * a.ldS);
      acc.x = ok ? acc.x + v.x : acc.x; acc.y = ok ? acc.y + v.y : acc.y; acc.z = ok ? acc.z + v.z : acc.z; acc.w = ok ? acc.w + v.w : acc.w;
    };
    const int* e = a.ell + r * a.W;
    for (int w0 = 0; w0 < a.W; w0 += 4) {
      const int4 id = *reinterpret_cast<const int4*>(e + w0);
      if ((id.x & id.y & id.z & id.w) < 0) continue;         // four empty entries
      add(id.x); add(id.y); add(id.z); add(id.w);
    }
    if (a.tail_ptr) {
      const int cap = (int)a.tail_cap;
      const int e_lo = cc_clamp(a.tail_ptr[r], 0, cap), e_hi = cc_clamp(a.tail_ptr[r + 1], e_lo, cap);
      for (int t = e_lo; t < e_hi; ++t) add(a.tail_col[t]);
    }
  }
  *reinterpret_cast<float4*>(a.out + r * a.ldo + 4 * q) = acc;
}

// ---------------------------------------------------------------- the backward
struct CapBwd {
  const float* S; int64_t ldS; const float* Z; int64_t ldZ; const float* AS; int64_t ldAS;
  const float* dxo; const float* dao;            // [B, K, F], [B, K, K]
  const int* graph_ptr; int B, K, F; int64_t row_cap, rows;
  float* dZ; int64_t lddZ; float* dS; int64_t lddS;
  const float* ro_dout; int64_t ro_ldo; const int* ro_arg;   // nullable: dZ += the max readout's gradient (dout [B, F], arg = winning row)
  int split;
};

// acc += A[32 x depth] . B[depth x 32] over `ngroups` groups of 8 contracted indices; load(g, av, bv) hands lane (i, h) the four
// values k = 8 g + 4 h .. + 3 of A's row i and of B's column i (zeros beyond the depth, from clamped addresses: a predicated load
// would be waited for on its own).  Four groups (sixteen MFMAs) per round, the next round's operands requested before the chain of
// this one issues: one wave per SIMD, nothing else hides the L2 latency.
template <class Load>
__device__ __forceinline__ void cc_chain(cc_f32x16& acc, int ngroups, Load load) {
  constexpr int U = 4;
  float4 a0[U], b0[U], a1[U], b1[U];
  auto fetch = [&](int g0, float4 (&av)[U], float4 (&bv)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) load(g0 + u, av[u], bv[u]);
  };
  auto run = [&](const float4 (&av)[U], const float4 (&bv)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u].x, bv[u].x, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u].y, bv[u].y, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u].z, bv[u].z, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u].w, bv[u].w, acc, 0, 0, 0);
    }
  };
  fetch(0, a0, b0);
  for (int g0 = 0; g0 < ngroups; g0 += 2 * U) {
    fetch(g0 + U, a1, b1);
    run(a0, b0);
    fetch(g0 + 2 * U, a0, b0);
    if (g0 + U < ngroups) run(a1, b1);
  }
}

__global__ __launch_bounds__(256) void contract_cap_bwd_kernel(CapBwd a) {
  const int tid = threadIdx.x, lane = tid & 63, i = lane & 31, h = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int K = a.K, F = a.F, cap = (int)a.row_cap;
  // the walk: which graph's rows hold slab number s, and where the batch ends.  Boundaries are clamped into [0, row_cap] and kept
  // monotone, so no word of graph_ptr can send a store outside the buffers.
  const int s = (int)blockIdx.x / a.split, part = (int)blockIdx.x - s * a.split;
  int lo = cc_clamp(a.graph_ptr[0], 0, cap), nslab = 0, b = -1, r0 = 0, r1 = 0;
  for (int k = 0; k < a.B; ++k) {
    const int hi = cc_clamp(a.graph_ptr[k + 1], lo, cap);
    const int ns = (hi - lo + 31) >> 5;
    if (s >= nslab && s < nslab + ns) { b = k; r0 = lo + 32 * (s - nslab); r1 = min(r0 + 32, hi); }
    nslab += ns;
    lo = hi;
  }
  const int n_tot = lo;
  if (b < 0) {
    // beyond the batch's slabs: the zero crew.  Two rows per pass, 128 threads a row: F / 4 + K / 4 <= 128 float4.
    const int zi = (int)blockIdx.x - nslab * a.split, crew = (int)gridDim.x - nslab * a.split;
    const int F4 = F >> 2, K4 = K >> 2, t = tid & 127;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t r = (int64_t)n_tot + 2 * zi + (tid >> 7); r < a.rows; r += 2 * (int64_t)crew) {
      if (t < F4) st_out(reinterpret_cast<float4*>(a.dZ + r * a.lddZ + 4 * t), zero4);
      else if (t < F4 + K4) st_out(reinterpret_cast<float4*>(a.dS + r * a.lddS + 4 * (t - F4)), zero4);
    }
    return;
  }
  const int nr = r1 - r0;
  const int64_t rowc = min(r0 + i, r1 - 1);                 // rows of the tile beyond the slab: a mapped row, their results are not kept
  const float* dxb = a.dxo + (int64_t)b * K * F;
  const float* dab = a.dao + (int64_t)b * K * K;
  const int njS = (K + 31) >> 5, njZ = (F + 31) >> 5;
  for (int j = part * 4 + wid; j < njS + njZ; j += 4 * a.split) {     // (uniform over the wave)
    cc_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float* out;
    int64_t ldo;
    int t, ncols, ra = -1;
    float rd = 0.f;
    if (j < njS) {
      // dS tile: Z . dX'^T (depth F), then AS . (dA' + dA'^T) (depth K)
      t = j; ncols = K; out = a.dS; ldo = a.lddS;
      const int nc = min(32 * t + i, K - 1);                // columns beyond K: a mapped column, not kept
      const float* zrow = a.Z + rowc * a.ldZ;
      const float* xrow = dxb + (int64_t)nc * F;
      cc_chain(acc, (F + 7) >> 3, [&](int g, float4& av, float4& bv) {
        const int k0 = 8 * g + 4 * h;
        const bool ok = k0 < F;
        const int kc = ok ? k0 : 0;
        const float4 ta = *reinterpret_cast<const float4*>(zrow + kc), tb = *reinterpret_cast<const float4*>(xrow + kc);
        av = cc_keep(ok, ta); bv = cc_keep(ok, tb);
      });
      const float* prow = a.AS + rowc * a.ldAS;
      const float* arow = dab + (int64_t)nc * K;
      const float* acol = dab + nc;
      cc_chain(acc, (K + 7) >> 3, [&](int g, float4& av, float4& bv) {
        const int k0 = 8 * g + 4 * h;
        const bool ok = k0 < K;
        const int kc = ok ? k0 : 0;
        const float4 ta = *reinterpret_cast<const float4*>(prow + kc), tt = *reinterpret_cast<const float4*>(arow + kc);
        const float* d = acol + (int64_t)kc * K;
        const float4 tb = make_float4(d[0] + tt.x, d[K] + tt.y, d[2 * K] + tt.z, d[3 * K] + tt.w);
        av = cc_keep(ok, ta); bv = cc_keep(ok, tb);
      });
    } else {
      // dZ tile: S . dX' (depth K)
      t = j - njS; ncols = F; out = a.dZ; ldo = a.lddZ;
      const int nc = min(32 * t + i, F - 1);
      if (a.ro_arg) { ra = a.ro_arg[(int64_t)b * F + nc]; rd = a.ro_dout[(int64_t)b * a.ro_ldo + nc]; }
      const float* srow = a.S + rowc * a.ldS;
      const float* xcol = dxb + nc;
      cc_chain(acc, (K + 7) >> 3, [&](int g, float4& av, float4& bv) {
        const int k0 = 8 * g + 4 * h;
        const bool ok = k0 < K;
        const int kc = ok ? k0 : 0;
        const float4 ta = *reinterpret_cast<const float4*>(srow + kc);
        const float* d = xcol + (int64_t)kc * F;
        const float4 tb = make_float4(d[0], d[F], d[2 * F], d[3 * F]);
        av = cc_keep(ok, ta); bv = cc_keep(ok, tb);
      });
    }
    const int c = 32 * t + i;
    if (c < ncols) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = (r & 3) + 8 * (r >> 2) + 4 * h;
        // (a winner outside this graph's real rows — its ghost row — matches no row stored here: discarded, as the caller expects)
        if (m < nr) st_out(out + (int64_t)(r0 + m) * ldo + c, acc[r] + ((r0 + m) == ra ? rd : 0.f));
      }
    }
  }
}

inline bool cc_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

/* see include/tsgnn.h */
int tsgnn_contract_cap_supported(int K, int F) {
  return (K >= 4 && K <= CC_KMAX && K % 4 == 0 && F >= 4 && F <= CC_FMAX && F % 4 == 0) ? 1 : 0;
}

int tsgnn_contract_cap_slabs(int64_t row_cap, int B) {
  if (row_cap < 0 || B < 1 || B > CC_MAX_B) return TSGNN_EINVAL;
  const int64_t n = ceil_div64(row_cap, 32) + B;
  return n > (int64_t)0x7fffffff / 4 ? TSGNN_EUNSUPPORTED : (int)n;
}

int tsgnn_ell_rowsum_f32(const int* ell, int W, const int* tail_ptr, const int* tail_col, int64_t tail_cap, const int* graph_ptr, int B,
                         int64_t row_cap, int nmax, const float* S, int64_t ldS, int K, float* out, int64_t ldo, tsgnn_stream_t stream) {
  if (!ell || !graph_ptr || !S || !out || (tail_ptr == nullptr) != (tail_col == nullptr) || (tail_ptr && tail_cap < 1)) return TSGNN_EINVAL;
  if (B < 1 || B > CC_MAX_B || row_cap <= 0 || nmax <= 0 || (W != 4 && W != 8 && W != 16) || K <= 0) return TSGNN_EINVAL;
  if (K > CC_KMAX || K % 4 || ldS < K || ldo < K || (ldS % 4) || (ldo % 4) || !cc_al16(ell) || !cc_al16(S) || !cc_al16(out))
    return TSGNN_EUNSUPPORTED;
  const int64_t rows = row_cap + nmax;
  if (rows >= ((int64_t)1 << 31) / 16 || tail_cap >= ((int64_t)1 << 31)) return TSGNN_EUNSUPPORTED;
  RowSum a{ell, W, tail_ptr, tail_col, tail_ptr ? tail_cap : 0, graph_ptr, B, row_cap, rows, S, ldS, K / 4, out, ldo};
  TSGNN_KNAME("ell_rowsum_kernel");
  ell_rowsum_kernel<<<(unsigned)ceil_div64(rows, 8), 256, 0, stream>>>(a);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

int tsgnn_contract_cap_bwd_f32(const float* S, int64_t ldS, const float* Z, int64_t ldZ, const float* AS, int64_t ldAS, const float* dxo,
                               const float* dao, const int* graph_ptr, int B, int K, int F, int64_t row_cap, int nmax, float* dZ,
                               int64_t lddZ, float* dS, int64_t lddS, const float* ro_dout, int64_t ro_ldo, const int* ro_arg, int split,
                               tsgnn_stream_t stream) {
  if (!S || !Z || !AS || !dxo || !dao || !graph_ptr || !dZ || !dS) return TSGNN_EINVAL;
  if (B < 1 || B > CC_MAX_B || row_cap <= 0 || nmax <= 0 || split < 0 || split > 4) return TSGNN_EINVAL;
  if ((ro_dout == nullptr) != (ro_arg == nullptr) || (ro_arg && ro_ldo < F)) return TSGNN_EINVAL;
  if (!tsgnn_contract_cap_supported(K, F)) return TSGNN_EUNSUPPORTED;
  if ((ldS % 4) || (ldZ % 4) || (ldAS % 4) || (lddZ % 4) || (lddS % 4) || ldS < K || ldAS < K || lddS < K || ldZ < F || lddZ < F ||
      !cc_al16(S) || !cc_al16(Z) || !cc_al16(AS) || !cc_al16(dxo) || !cc_al16(dao) || !cc_al16(dZ) || !cc_al16(dS))
    return TSGNN_EUNSUPPORTED;
  const int64_t rows = row_cap + nmax;
  const int slabs = tsgnn_contract_cap_slabs(row_cap, B);
  if (rows >= ((int64_t)1 << 31) || slabs < 0) return TSGNN_EUNSUPPORTED;
  if (split == 0) {
    // one tile per wave where the slab has that many (K = 100, F = 384: 4 + 12 tiles, four workgroups); measured: profiles/r15
    const int jobs = (K + 31) / 32 + (F + 31) / 32;
    split = jobs > 12 ? 4 : (jobs + 3) / 4;
  }
  CapBwd a{S, ldS, Z, ldZ, AS, ldAS, dxo, dao, graph_ptr, B, K, F, row_cap, rows, dZ, lddZ, dS, lddS, ro_dout, ro_ldo, ro_arg, split};
  TSGNN_KNAME("contract_cap_bwd_kernel");
  contract_cap_bwd_kernel<<<(unsigned)(slabs * split + CC_ZERO_BLOCKS), 256, 0, stream>>>(a);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
