// The protocol every stream's gather launch shares (triplet_stream, batch_stream, sag_stream, sag_batch_stream, gat_stream,
// eigen_stream): one [HEAD | schedule] buffer per stream, HEAD = state {cursor, T} as two int64 + the ticket counter (the streams of up
// to 128 graphs per entry keep 32 shards + a top counter in a tensor of their own), then T entries of B graph indices.  A launch
// reads "entry number cursor mod T"; its last workgroup to draw a ticket advances the cursor.  Nobody waits for anybody, and the
// ticket words are the launch's only atomics.
//
// Order inside a workgroup: the first B threads call stream_entry_id (thread 0 leaves the cursor it read in LDS), a barrier follows,
// and only behind that barrier thread 0 draws the workgroup's ticket — so the workgroup that draws the last ticket knows that EVERY
// workgroup has read the cursor, and may overwrite it.
#pragma once
#include "common.h"

constexpr int STREAM_MAX_B = 128;         // graphs per entry of the two-wave prologue (two_wave_prefix)
constexpr int STREAM_SHARDS = 32, STREAM_SHARD_WORDS = 32;     // sharded ticket: 32 shards + the top, each on 128 bytes of its own

// Thread tid < B: the graph its word of the cursor's schedule entry names, clamped into [0, n_graphs) — load() validated the
// schedule, and a stale or overwritten word still never leaves the records.  cur_out: the cursor as read.
__device__ __forceinline__ int64_t stream_entry_id(int64_t* state, const int32_t* sched, int64_t sched_cap, int64_t n_graphs, int B, int tid,
                                                   long long& cur_out) {
  // (agent-scope load: the word is stored by the last workgroup of the previous launch, never through this CU's scalar cache)
  const long long cur = __hip_atomic_load(reinterpret_cast<long long*>(state), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  int64_t T = state[1];                                     // the loaded schedule's length: the host's word, kept inside the buffer
  T = T < 1 ? 1 : (T > sched_cap ? sched_cap : T);
  const int64_t c = (int64_t)((unsigned long long)cur % (unsigned long long)T);
  const int64_t id = sched[c * B + tid];
  cur_out = cur;
  return id < 0 ? 0 : (id >= n_graphs ? n_graphs - 1 : id);
}

// Thread 0, behind the barrier: one counter for the whole grid.  The workgroup that draws the last of n_workgroups tickets leaves the
// counter at zero for the next launch and advances the cursor.
__device__ __forceinline__ void stream_ticket_flat(unsigned* ticket, unsigned n_workgroups, int64_t* state, long long cur) {
  const unsigned t = atomicAdd(ticket, 1u);
  if (t == n_workgroups - 1) {
    atomicExch(ticket, 0u);
    __hip_atomic_store(reinterpret_cast<long long*>(state), cur + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Thread 0, behind the barrier, for a 1-D grid of a thousand workgroups and more.  Atomics execute at the memory side, one after the
// other on one line, so the tickets are drawn in two levels: workgroup b draws from shard b % 32 (a counter on 128 bytes of its own);
// the workgroup that draws a shard's last ticket leaves the shard at zero and draws from the top counter; the one that draws the top's
// last knows that all have read the cursor, leaves the top at zero and advances the cursor.
__device__ __forceinline__ void stream_ticket_sharded(unsigned* ticket, int64_t* state, long long cur) {
  const unsigned S = gridDim.x < (unsigned)STREAM_SHARDS ? gridDim.x : (unsigned)STREAM_SHARDS;
  const unsigned s = blockIdx.x % S;
  const unsigned members = (gridDim.x - s + S - 1) / S;     // workgroups b < gridDim.x with b % S == s
  unsigned* shard = ticket + s * STREAM_SHARD_WORDS;
  if (atomicAdd(shard, 1u) == members - 1) {
    atomicExch(shard, 0u);
    unsigned* top = ticket + STREAM_SHARDS * STREAM_SHARD_WORDS;
    if (atomicAdd(top, 1u) == S - 1) {
      atomicExch(top, 0u);
      __hip_atomic_store(reinterpret_cast<long long*>(state), cur + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// inclusive prefix sum over the 64 lanes of a wave
__device__ __forceinline__ int wave_scan_inclusive(int v, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(v, d, 64);
    if (lane >= d) v += u;
  }
  return v;
}

// Every thread of the workgroup (two barriers inside): the exclusive prefix sums pre_a / pre_b [STREAM_MAX_B + 1] of two quantities
// that threads [0, STREAM_MAX_B) hold — waves 0 and 1, whole waves; threads past B carry zeros.  Wave 1 adds wave 0's total through
// wtot [2][2].
__device__ __forceinline__ void two_wave_prefix(int va, int vb, int tid, int (*wtot)[2], int* pre_a, int* pre_b) {
  const int lane = tid & 63, wave = tid >> 6;
  if (tid < STREAM_MAX_B) {
    va = wave_scan_inclusive(va, lane);
    vb = wave_scan_inclusive(vb, lane);
    if (lane == 63) { wtot[wave][0] = va; wtot[wave][1] = vb; }
  }
  __syncthreads();
  if (tid == 0) {
    pre_a[0] = 0; pre_b[0] = 0;
  }
  if (tid < STREAM_MAX_B) {
    pre_a[tid + 1] = va + (wave ? wtot[0][0] : 0);
    pre_b[tid + 1] = vb + (wave ? wtot[0][1] : 0);
  }
  __syncthreads();
}
