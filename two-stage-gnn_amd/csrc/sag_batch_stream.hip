// SAGPool mini-batch stream: a NEW mini-batch of B graphs every replay of one hipGraph (Code/sag/train.py:181-198: DataLoader(batch_size
// = 128, shuffle=True) -> F.nll_loss(model(data), data.y) -> Adam, once per optimiser step), for sag_layers.Net(use_batch=True).
// csrc/sag_stream.hip writes what sag_stack's node reads of 3 graphs (or 1); this is that launch for entries of 1 <= B <= 128 graphs,
// with the B-graph machinery of csrc/batch_stream.hip: the same arena (sag_stream.pack_arena), the same [HEAD | schedule] buffer with
// its cursor, the same per-row body, and
//
//   prologue   the first B threads load the entry's records; the first two waves form the inclusive prefix sums of n and nnz with
//              wave shuffles (wave 1 adds wave 0's total through LDS)
//   per row    8 lanes per row, 32 rows per workgroup; a binary search over the prefix (at most 7 LDS reads, the same address in all
//              lanes of a row) finds the row's graph, one 16-byte LDS read fetches that graph's offsets
//   workgroup 0   ids_out [B], label_out [B] (int64: what mp.nll_loss folds into the head's backward) and the graph pointer of EVERY
//              level, gp [depth + 1][ldg]: one thread per graph applies k = min(n, ceilf(ratio * (float)n)) level after level, an LDS
//              scan per level forms the prefix, every word is clamped to its level's capacity, words past B repeat the total
//
// The capacities may lie below B times the largest graph (sag_stream.MiniBatchStream.load checks every entry on the host): for an entry
// that does not fit, rows and entries past the capacities are dropped and every pointer is clamped, so nothing is written outside the
// arrays.  One writer per word, plain vector stores (16 bytes wherever sag_stream.hip has them), and the ticket words of
// batch_stream.hip (32 shards + the top, 128 bytes each) are the only atomics.
#include "common.h"
#include "../../include/tsgnn.h"

namespace {

constexpr int SB_MAX_B = 128;
constexpr int SB_SHARDS = 32, SB_SHARD_WORDS = 32;       // ticket counters: 32 shards + the top, each on 128 bytes of its own
constexpr int SB_REC = 8;                 // int32 words of a record: n, nnz, first row, first entry, index, 0, 0, 0
constexpr int SB_MAX_DEPTH = 7;
constexpr int SB_EG = 8;                  // lanes per row
constexpr int SB_ROWS = 256 / SB_EG;      // rows per workgroup

struct SagBatchGatherArgs {
  const int32_t* rec; int64_t n_graphs;
  const int32_t *rowptr, *col;            // the arena's sections: graph g's n + 1 row pointers (graph-local) start at first row + g
  const float* feats; int64_t ldf; int ld4;
  const int32_t* labels;                  // [n_graphs]
  const int32_t* sched; int64_t sched_cap; int64_t* state; unsigned* ticket;      // state = {cursor, T}
  int B; int64_t row_cap, nnz_cap; float ratio; int depth; int ldg;
  int32_t level_cap[SB_MAX_DEPTH + 1];
  int32_t *rowptr_out, *col_out; float* x; int64_t ldx; float *dinv, *self_w; int32_t *gp, *ids_out; int64_t* label_out;
};

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ int sb_wave_scan(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

__global__ __launch_bounds__(256) void sag_batch_gather_kernel(SagBatchGatherArgs a) {
  __shared__ int4 off_s[SB_MAX_B];        // first row, first entry, id, 0
  __shared__ int pre_n[SB_MAX_B + 1], pre_e[SB_MAX_B + 1];      // exclusive prefix sums of n / nnz over the entry's graphs
  __shared__ int wtot_s[2][2];            // wave totals of n / nnz
  __shared__ int lvl_tot_s[SB_MAX_DEPTH + 1][2];                 // workgroup 0: wave totals of k^l(n)
  __shared__ int gp_s[SB_MAX_DEPTH + 1][SB_MAX_B + 4];           // workgroup 0: the graph pointers, before they go out 16 bytes a store
  __shared__ long long cur_s;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  int n_i = 0, e_i = 0;
  if (tid < a.B) {
    // (agent-scope load: the word is stored by the last workgroup of the previous launch, never through this CU's scalar cache)
    const long long cur = __hip_atomic_load(reinterpret_cast<long long*>(a.state), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int64_t T = a.state[1];                                 // the loaded schedule's length: the host's word, kept inside the buffer
    T = T < 1 ? 1 : (T > a.sched_cap ? a.sched_cap : T);
    const int64_t c = (int64_t)((unsigned long long)cur % (unsigned long long)T);
    int64_t id = a.sched[c * a.B + tid];
    id = id < 0 ? 0 : (id >= a.n_graphs ? a.n_graphs - 1 : id);      // (load() validated it; an index never leaves the records)
    const int4 r0 = *reinterpret_cast<const int4*>(a.rec + id * SB_REC);
    n_i = r0.x; e_i = r0.y;
    off_s[tid] = make_int4(r0.z, r0.w, (int)id, 0);
    if (tid == 0) cur_s = cur;
    if (blockIdx.x == 0) {                                  // the batch's own small arrays: one writer per word
      a.ids_out[tid] = (int32_t)id;
      a.label_out[tid] = (int64_t)a.labels[id];
    }
  }
  int sn = n_i, se = e_i;
  if (tid < SB_MAX_B) {                                     // waves 0 and 1, whole waves: threads past B carry zeros
    sn = sb_wave_scan(sn, lane);
    se = sb_wave_scan(se, lane);
    if (lane == 63) { wtot_s[wave][0] = sn; wtot_s[wave][1] = se; }
  }
  __syncthreads();
  if (tid == 0) {
    pre_n[0] = 0; pre_e[0] = 0;
  }
  if (tid < SB_MAX_B) {
    pre_n[tid + 1] = sn + (wave ? wtot_s[0][0] : 0);
    pre_e[tid + 1] = se + (wave ? wtot_s[0][1] : 0);
  }
  __syncthreads();

  const int n_tot = pre_n[a.B], e_tot = pre_e[a.B];
  // (an entry that fits never reaches the clamps; one that does not — refused by the host's load — leaves pointers inside col)
  const int e_end = (int)((int64_t)e_tot < a.nnz_cap ? (int64_t)e_tot : a.nnz_cap);
  if (blockIdx.x == 0) {                                    // (uniform over the workgroup: the barriers below are met by every thread)
    // level l's graph pointer: thread b holds k^l(n_b) (threads past B: 0, so their words repeat the total), an LDS scan per level
    int s = n_i;
    for (int l = 0; l <= a.depth; ++l) {
      int sc = 0;
      if (tid < SB_MAX_B) {
        sc = sb_wave_scan(s, lane);
        if (lane == 63) lvl_tot_s[l][wave] = sc;
      }
      __syncthreads();
      if (tid < SB_MAX_B) {
        const int p = sc + (wave ? lvl_tot_s[l][0] : 0);
        gp_s[l][tid + 1] = p < a.level_cap[l] ? p : a.level_cap[l];
      }
      if (tid == 0) gp_s[l][0] = 0;
      const int kk = (int)ceilf(a.ratio * (float)s);        // float32, as PyG's topk and SagPlan compute it
      s = kk < s ? kk : s;
    }
    __syncthreads();
    const int q4 = a.ldg >> 2;
    for (int i = tid; i < (a.depth + 1) * q4; i += 256) {
      const int l = i / q4, j = 4 * (i - l * q4);
      const int* g = gp_s[l];                               // (B <= 128: word 128 is the total whatever B)
      const int j1 = j + 1 < SB_MAX_B ? j + 1 : SB_MAX_B, j2 = j + 2 < SB_MAX_B ? j + 2 : SB_MAX_B, j3 = j + 3 < SB_MAX_B ? j + 3 : SB_MAX_B;
      *reinterpret_cast<int4*>(a.gp + (int64_t)l * a.ldg + j) = make_int4(g[j < SB_MAX_B ? j : SB_MAX_B], g[j1], g[j2], g[j3]);
    }
    if (tid == 64) a.rowptr_out[a.row_cap] = e_end;
  }

  const int64_t r = (int64_t)blockIdx.x * SB_ROWS + (tid >> 3);
  const int sub = tid & (SB_EG - 1);
  // the graph whose rows hold r: the last k with pre_n[k] <= r (every graph has a row, so the prefix is strictly increasing); a trip
  // count that depends on B alone
  int lo = 0, hi = a.B;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((int64_t)pre_n[mid] <= r) lo = mid; else hi = mid;
  }
  const bool in_cap = r < a.row_cap;
  const bool real = r < (int64_t)n_tot && in_cap;
  const int b = lo;
  const int g0 = pre_n[b], eb = pre_e[b];
  const int4 o4 = off_s[b];
  const int row0 = o4.x, ent0 = o4.y, gid = o4.z;
  const int lr = (int)(r - g0);
  int e0 = 0, e1 = 0;
  if (real) {
    const int32_t* rp = a.rowptr + (int64_t)row0 + gid + lr;
    e0 = rp[0]; e1 = rp[1];
  }
  bool has_self = false;
  for (int e = e0 + sub; e < e1; e += SB_EG) {
    const int c = a.col[(int64_t)ent0 + e];
    has_self |= (c == lr);
    const int64_t o = (int64_t)eb + e;
    if (o < a.nnz_cap) a.col_out[o] = c + g0;
  }
  // (every lane of the wave is here: rows past row_cap only skip their stores)
  has_self = ((unsigned)(__ballot(has_self) >> (lane & ~(SB_EG - 1))) & ((1u << SB_EG) - 1u)) != 0u;
  float di = 0.f, sw = 0.f;
  if (real) gcn_norm_coef(e1 - e0, has_self, di, sw);
  int rp_out = real ? eb + e0 : e_tot;
  rp_out = rp_out < e_end ? rp_out : e_end;
  {
    const int q0 = lane & ~31;                              // the 32-lane group's first lane: rows r .. r + 3 of a multiple of four
    const int4 rp4 = make_int4(rp_out, __shfl(rp_out, q0 + 8, 64), __shfl(rp_out, q0 + 16, 64), __shfl(rp_out, q0 + 24, 64));
    const float4 di4 = make_float4(di, __shfl(di, q0 + 8, 64), __shfl(di, q0 + 16, 64), __shfl(di, q0 + 24, 64));
    const float4 sw4 = make_float4(sw, __shfl(sw, q0 + 8, 64), __shfl(sw, q0 + 16, 64), __shfl(sw, q0 + 24, 64));
    if ((tid & 31) == 0 && in_cap) {
      if (r + 3 < a.row_cap) {
        *reinterpret_cast<int4*>(a.rowptr_out + r) = rp4;
        *reinterpret_cast<float4*>(a.dinv + r) = di4;
        *reinterpret_cast<float4*>(a.self_w + r) = sw4;
      } else {                                              // the last rows of a capacity that is no multiple of four
        const int rp_[4] = {rp4.x, rp4.y, rp4.z, rp4.w};
        const float di_[4] = {di4.x, di4.y, di4.z, di4.w}, sw_[4] = {sw4.x, sw4.y, sw4.z, sw4.w};
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (r + u < a.row_cap) {
            a.rowptr_out[r + u] = rp_[u];
            a.dinv[r + u] = di_[u];
            a.self_w[r + u] = sw_[u];
          }
      }
    }
  }
  if (in_cap) {
    const float4* src = reinterpret_cast<const float4*>(a.feats + ((int64_t)row0 + lr) * a.ldf);
    for (int c4 = sub; c4 < a.ld4; c4 += SB_EG) {
      const float4 v = real ? src[c4] : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(a.x + r * a.ldx + 4 * c4) = v;
    }
  }
  // This workgroup READ the cursor before its first barrier (the value went through LDS), so thread 0 may draw the workgroup's ticket;
  // here, behind its stores, so that no wave waits for the atomic's round trip in front of its work.  Two levels, as in
  // batch_stream.hip (a DD-shaped batch of 128 graphs has more than 1,400 workgroups): workgroup b draws from shard b % 32; the one
  // that draws a shard's last ticket leaves the shard at zero and draws from the top counter; the one that draws the top's last knows
  // that all have read the cursor, leaves the top at zero and advances the cursor.  Nobody waits for anybody.
  if (tid == 0) {
    const long long cur = cur_s;
    const unsigned S = gridDim.x < (unsigned)SB_SHARDS ? gridDim.x : (unsigned)SB_SHARDS;
    const unsigned s = blockIdx.x % S;
    const unsigned members = (gridDim.x - s + S - 1) / S;   // workgroups b < gridDim.x with b % S == s
    unsigned* shard = a.ticket + s * SB_SHARD_WORDS;
    if (atomicAdd(shard, 1u) == members - 1) {
      atomicExch(shard, 0u);
      unsigned* top = a.ticket + SB_SHARDS * SB_SHARD_WORDS;
      if (atomicAdd(top, 1u) == S - 1) {
        atomicExch(top, 0u);
        __hip_atomic_store(reinterpret_cast<long long*>(a.state), cur + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
}

}  // namespace

extern "C" {

/* see include/tsgnn.h */
int tsgnn_sag_batch_gather_f32(const int32_t* records, int64_t n_graphs, const int32_t* arena, int64_t off_rowptr, int64_t off_col,
                               int64_t arena_words, const float* feats, int64_t ldf, const int32_t* labels, int64_t max_n,
                               int64_t max_nnz, const int32_t* sched, int64_t sched_cap, int64_t* state, unsigned* ticket, int B,
                               int64_t row_cap, int64_t nnz_cap, const int64_t* level_caps, float ratio, int depth, int32_t* rowptr,
                               int32_t* col, float* x, int64_t ldx, float* dinv, float* self_w, int32_t* graph_ptr, int64_t ldg,
                               int32_t* ids_out, int64_t* label_out, tsgnn_stream_t stream) {
  if (!records || !arena || !feats || !labels || !sched || !state || !ticket || !level_caps || !rowptr || !col || !x || !dinv || !self_w ||
      !graph_ptr || !ids_out || !label_out)
    return TSGNN_EINVAL;
  if (B < 1 || B > SB_MAX_B || sched_cap <= 0 || n_graphs <= 0 || row_cap <= 0 || nnz_cap < 1 || ldf <= 0 || max_n < 1 || max_nnz < 0 ||
      depth < 1 || depth > SB_MAX_DEPTH || !(ratio > 0.f) || !(ratio <= 1.f))
    return TSGNN_EINVAL;
  if (ldg < B + 1 || (ldg % 4)) return TSGNN_EINVAL;
  if (off_rowptr < 0 || off_col < off_rowptr || arena_words < off_col) return TSGNN_EINVAL;
  if (max_n >= ((int64_t)1 << 31) / B || max_nnz >= ((int64_t)1 << 31) / B || row_cap >= ((int64_t)1 << 31) - SB_ROWS ||
      nnz_cap >= ((int64_t)1 << 31) || sched_cap >= ((int64_t)1 << 31) / B || ldg >= ((int64_t)1 << 31) / (SB_MAX_DEPTH + 1))
    return TSGNN_EUNSUPPORTED;
  // every graph of the arena fits the slot on its own at every level (max_n and max_nnz are the caller's word, as the arena is).
  // Whether an ENTRY fits is the uploader's check (sag_stream.MiniBatchStream.load): the kernel clamps, so an entry that does not fit
  // cannot write outside the arrays.
  if (row_cap < max_n || nnz_cap < max_nnz || level_caps[0] != row_cap) return TSGNN_EINVAL;
  SagBatchGatherArgs a{};
  {
    int s = (int)max_n;
    for (int l = 0; l <= depth; ++l) {
      if (level_caps[l] < s) return TSGNN_EINVAL;
      if (level_caps[l] >= ((int64_t)1 << 31)) return TSGNN_EUNSUPPORTED;
      a.level_cap[l] = (int32_t)level_caps[l];
      const int kk = (int)ceilf(ratio * (float)s);
      s = kk < s ? kk : s;
    }
  }
  if ((ldf % 4) || ldx != ldf || ((off_rowptr | off_col) & 3)) return TSGNN_EUNSUPPORTED;
  const uintptr_t al = reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(arena) | reinterpret_cast<uintptr_t>(feats) |
                       reinterpret_cast<uintptr_t>(rowptr) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(dinv) |
                       reinterpret_cast<uintptr_t>(self_w) | reinterpret_cast<uintptr_t>(graph_ptr) | reinterpret_cast<uintptr_t>(state);
  if ((al & 15) || (reinterpret_cast<uintptr_t>(label_out) & 7)) return TSGNN_EUNSUPPORTED;
  a.rec = records; a.n_graphs = n_graphs; a.rowptr = arena + off_rowptr; a.col = arena + off_col;
  a.feats = feats; a.ldf = ldf; a.ld4 = (int)(ldf / 4); a.labels = labels;
  a.sched = sched; a.sched_cap = sched_cap; a.state = state; a.ticket = ticket;
  a.B = B; a.row_cap = row_cap; a.nnz_cap = nnz_cap; a.ratio = ratio; a.depth = depth; a.ldg = (int)ldg;
  a.rowptr_out = rowptr; a.col_out = col; a.x = x; a.ldx = ldx; a.dinv = dinv; a.self_w = self_w; a.gp = graph_ptr; a.ids_out = ids_out;
  a.label_out = label_out;
  TSGNN_KNAME("sag_batch_gather_kernel");
  sag_batch_gather_kernel<<<(unsigned)ceil_div64(row_cap, SB_ROWS), 256, 0, stream>>>(a);
  TSGNN_CHECK_LAUNCH();
  return TSGNN_OK;
}

}  // extern "C"
