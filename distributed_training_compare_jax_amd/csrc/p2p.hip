// Peer-to-peer all-reduce over xGMI for the latency-bound tensor-parallel messages
// (4 all-reduces of the [tokens, d_model] fp32 residual per layer).
//
// Every rank allocates one uncached device buffer, exports it with hipIpcGetMemHandle and maps
// every peer's buffer (hipIpcOpenMemHandle), so a kernel on rank r can load any peer's memory
// directly over the point-to-point xGMI links — all 7 links of an 8-GPU node at once, instead
// of the one outgoing link a ring step uses.  The all-reduce is two-shot:
//
//   copy   x -> own buffer half (h = call parity)
//   barrier
//   reduce-scatter: rank r sums slice r of every peer's half h, in rank order, into its own half
//   barrier
//   all-gather: out[slice q] = peer q's reduced slice (own slice local)
//
// so each rank moves 2(W-1)/W of the message over xGMI, and every rank computes the SAME sum in
// the SAME order (bitwise identical replicas).  Alternating halves makes a third barrier
// unnecessary: call k+2 rewrites half h only after passing call k+1's barriers, which every rank
// reaches only after finishing call k.
//
// Barriers: rank r stores the epoch into flags[r] of every peer (system-scope release) and spins
// on its own flags[p] >= epoch (system-scope acquire).  The epoch is a device counter, so the
// whole sequence is plain stream-ordered kernels that hipGraph capture records like any other
// kernel (no graph cut, unlike an eager RCCL call).  Every spin is bounded: after ~10 s it sets
// an error word and exits, so a missing peer shows up as an error, never as a hung GPU.
#include "common.h"
#include <algorithm>
#include <cstring>
#include <type_traits>

namespace {

constexpr int P2P_MAX = 8;
constexpr int FLAG_BYTES = 4096;  // flag area at the start of each buffer (epoch per source rank)

struct PeerTable {
  unsigned char* base[P2P_MAX];  // buffer base of every rank (own included), as mapped here
};

__device__ __forceinline__ uint64_t wall_clock() { return __builtin_amdgcn_s_memrealtime(); }  // 100 MHz

// inc: 1 per barrier of the two-shot call (2 barriers), 2 for the one-shot call's single barrier, so
// every call advances the epoch by 2 and the buffer half stays (epoch >> 1) & 1 at the call's start
__global__ void p2p_barrier_kernel(PeerTable t, int rank, int world, uint32_t* __restrict__ epoch,
                                   int* __restrict__ err, int inc) {
  const int p = threadIdx.x;
  DTC_ASSERT(world >= 1 && world <= P2P_MAX && rank >= 0 && rank < world && (inc == 1 || inc == 2));
  const uint32_t e = epoch[0] + inc;
  __threadfence_system();  // this rank's prior writes (its buffer half) before the signal
  if (p < world && p != rank) {
    uint32_t* peer_flag = (uint32_t*)t.base[p] + rank;
    __hip_atomic_store(peer_flag, e, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    const uint32_t* mine = (const uint32_t*)t.base[rank] + p;
    const uint64_t t0 = wall_clock();
    while (__hip_atomic_load(mine, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < e) {
      __builtin_amdgcn_s_sleep(2);
      if (wall_clock() - t0 > 1000000000ull) {  // ~10 s at 100 MHz
        atomicExch(err, 1000 + p);
        break;
      }
    }
  }
  __syncthreads();
  if (p == 0) epoch[0] = e;
}

// copy x into own half h (h read from the epoch counter parity: 2 barriers per call)
__global__ void p2p_stage_kernel(const f32x4* __restrict__ x, PeerTable t, int rank, long n4, long half_bytes,
                                 const uint32_t* __restrict__ epoch) {
  const int h = (epoch[0] >> 1) & 1;
  DTC_ASSERT(16 * n4 <= half_bytes && rank >= 0);
  f32x4* dst = (f32x4*)(t.base[rank] + FLAG_BYTES + h * half_bytes);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) dst[i] = x[i];
}

__global__ void p2p_reduce_scatter_kernel(PeerTable t, int rank, int world, long n4, long half_bytes,
                                          const uint32_t* __restrict__ epoch) {
  const int h = ((epoch[0] - 1) >> 1) & 1;  // one barrier has passed since the stage
  const long chunk = (n4 + world - 1) / world;
  const long lo = rank * chunk, hi = min(n4, lo + chunk);
  const long off = FLAG_BYTES + h * half_bytes;
  DTC_ASSERT(16 * n4 <= half_bytes && rank < world);
  for (long i = lo + (long)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (long)gridDim.x * blockDim.x) {
    f32x4 s = ((const f32x4*)(t.base[0] + off))[i];
    for (int p = 1; p < world; ++p) s += ((const f32x4*)(t.base[p] + off))[i];
    ((f32x4*)(t.base[rank] + off))[i] = s;
  }
}

__global__ void p2p_all_gather_kernel(PeerTable t, int world, long n4, long half_bytes, f32x4* __restrict__ out,
                                      const uint32_t* __restrict__ epoch) {
  const int h = ((epoch[0] - 2) >> 1) & 1;
  const long chunk = (n4 + world - 1) / world;
  const long off = FLAG_BYTES + h * half_bytes;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const int q = (int)(i / chunk);
    DTC_ASSERT(q < world);
    out[i] = ((const f32x4*)(t.base[q] + off))[i];
  }
}

// one-shot (small messages): after the single barrier every rank sums ALL ranks' halves itself, in
// rank order (identical result on every rank); (W-1) n bytes over xGMI instead of 2 (W-1)/W n, but
// one barrier and two fewer launches: the latency path for the CE row statistics, label logits and
// the grad-norm scalar
__global__ void p2p_oneshot_kernel(PeerTable t, int world, long n4, long half_bytes, f32x4* __restrict__ out,
                                   const uint32_t* __restrict__ epoch) {
  const int h = ((epoch[0] - 2) >> 1) & 1;
  const long off = FLAG_BYTES + h * half_bytes;
  DTC_ASSERT(16 * n4 <= half_bytes && world >= 1);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 s = ((const f32x4*)(t.base[0] + off))[i];
    for (int p = 1; p < world; ++p) s += ((const f32x4*)(t.base[p] + off))[i];
    out[i] = s;
  }
}

// ---------------------------------------------------------------- bf16 payload (tp_comm_dtype: bf16)
// Row-parallel partials travel as bf16 (half the xGMI bytes of the fp32 residual), are summed in fp32
// in rank order, and the LAST kernel adds the fp32 residual and the bias:
//   out[i] = resid[i] + bias[i % ncols] + sum_p partial_p[i]
// so the residual stream itself is never rounded (only the layer's delta is, once, to bf16).  The
// two-shot reduce-scatter stores its reduced slice in bf16 (the all-gather reads half the bytes).
__global__ void p2p_stage_bf16_kernel(const bf16x8* __restrict__ x, PeerTable t, int rank, long n8, long half_bytes,
                                      const uint32_t* __restrict__ epoch) {
  const int h = (epoch[0] >> 1) & 1;
  DTC_ASSERT(16 * n8 <= half_bytes && rank >= 0);
  bf16x8* dst = (bf16x8*)(t.base[rank] + FLAG_BYTES + h * half_bytes);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) dst[i] = x[i];
}

__device__ __forceinline__ void add8(float (&a)[8], const bf16x8& v) {
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] += (float)v[e];
}

// out (fp32) = resid + bias + the 8 values a, for elements 8i .. 8i+7
__device__ __forceinline__ void finish8(float (&a)[8], long i, float* __restrict__ out, const float* __restrict__ resid,
                                        const float* __restrict__ bias, int ncols) {
  if (resid) {
    const f32x4 r0 = ((const f32x4*)resid)[2 * i], r1 = ((const f32x4*)resid)[2 * i + 1];
#pragma unroll
    for (int e = 0; e < 4; ++e) { a[e] += r0[e]; a[e + 4] += r1[e]; }
  }
  if (bias) {
    const int c0 = (int)((8 * i) % ncols);  // ncols % 8 == 0: the 8 columns share a row
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] += bias[c0 + e];
  }
  ((f32x4*)out)[2 * i] = f32x4{a[0], a[1], a[2], a[3]};
  ((f32x4*)out)[2 * i + 1] = f32x4{a[4], a[5], a[6], a[7]};
}

__global__ void p2p_oneshot_bf16_kernel(PeerTable t, int world, long n8, long half_bytes, float* __restrict__ out,
                                        const float* __restrict__ resid, const float* __restrict__ bias, int ncols,
                                        const uint32_t* __restrict__ epoch) {
  const int h = ((epoch[0] - 2) >> 1) & 1;
  const long off = FLAG_BYTES + h * half_bytes;
  DTC_ASSERT(16 * n8 <= half_bytes && world >= 1 && ncols % 8 == 0);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < world; ++p) add8(a, ((const bf16x8*)(t.base[p] + off))[i]);
    finish8(a, i, out, resid, bias, ncols);
  }
}

__global__ void p2p_reduce_scatter_bf16_kernel(PeerTable t, int rank, int world, long n8, long half_bytes,
                                               const uint32_t* __restrict__ epoch) {
  const int h = ((epoch[0] - 1) >> 1) & 1;
  const long chunk = (n8 + world - 1) / world;
  const long lo = rank * chunk, hi = min(n8, lo + chunk);
  const long off = FLAG_BYTES + h * half_bytes;
  DTC_ASSERT(16 * n8 <= half_bytes && rank < world);
  for (long i = lo + (long)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (long)gridDim.x * blockDim.x) {
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < world; ++p) add8(a, ((const bf16x8*)(t.base[p] + off))[i]);
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(a[e]);
    ((bf16x8*)(t.base[rank] + off))[i] = o;
  }
}

__global__ void p2p_all_gather_bf16_kernel(PeerTable t, int world, long n8, long half_bytes, float* __restrict__ out,
                                           const float* __restrict__ resid, const float* __restrict__ bias, int ncols,
                                           const uint32_t* __restrict__ epoch) {
  const int h = ((epoch[0] - 2) >> 1) & 1;
  const long chunk = (n8 + world - 1) / world;
  const long off = FLAG_BYTES + h * half_bytes;
  DTC_ASSERT(16 * n8 <= half_bytes && world >= 1 && ncols % 8 == 0);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    add8(a, ((const bf16x8*)(t.base[(int)(i / chunk)] + off))[i]);
    finish8(a, i, out, resid, bias, ncols);
  }
}

// ---------------------------------------------------------------- sequence parallelism (tp_sequence_parallel)
// The residual stream is split by rows over the TP ranks, so the row-parallel GEMMs' partial sums are
// REDUCE-SCATTERED (each rank only needs its own rows) and the LayerNorm outputs / residual gradients
// that feed the column-parallel GEMMs are ALL-GATHERED.  Both are one barrier each: the payload (the
// whole [rows, cols] partial, or this rank's slice at its row offset) is in every rank's buffer half
// before the barrier; afterwards rank r reads what it needs straight from the peers' halves.
//
// reduce-scatter: out[i] (fp32, this rank's n_loc elements) = resid[i] + bias[col] + sum_p partial_p[lo + i],
// summed in rank order (the same order on every rank: a row's value does not depend on who owns it)
template <bool BF16>
__global__ void p2p_rs_kernel(PeerTable t, int rank, int world, long n8_loc, long half_bytes, float* __restrict__ out,
                              const float* __restrict__ resid, const float* __restrict__ bias, int ncols,
                              const uint32_t* __restrict__ epoch) {
  const int h = ((epoch[0] - 2) >> 1) & 1;
  const long off = FLAG_BYTES + h * half_bytes;
  const long lo8 = (long)rank * n8_loc;
  DTC_ASSERT(rank < world && (BF16 ? 16 : 32) * n8_loc * world <= half_bytes && (!bias || ncols % 8 == 0));
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8_loc; i += (long)gridDim.x * blockDim.x) {
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < world; ++p) {
      if constexpr (BF16) {
        add8(a, ((const bf16x8*)(t.base[p] + off))[lo8 + i]);
      } else {
        const f32x4* src = (const f32x4*)(t.base[p] + off) + 2 * (lo8 + i);
        const f32x4 v0 = src[0], v1 = src[1];
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[e] += v0[e]; a[e + 4] += v1[e]; }
      }
    }
    finish8(a, i, out, resid, bias, ncols);  // i indexes this rank's rows: column = (8 i) % ncols
  }
}

// stage n16 16-byte pieces of x into own half at piece offset `at` (the all-gather's slot / a full partial)
__global__ void p2p_stage16_kernel(const u32x4* __restrict__ x, PeerTable t, int rank, long at, long n16,
                                   long half_bytes, const uint32_t* __restrict__ epoch) {
  const int h = (epoch[0] >> 1) & 1;
  DTC_ASSERT(16 * (at + n16) <= half_bytes && rank >= 0);
  u32x4* dst = (u32x4*)(t.base[rank] + FLAG_BYTES + h * half_bytes) + at;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x) dst[i] = x[i];
}

// all-gather: out[q * n16_loc + i] = rank q's slot (16-byte pieces, any element type); own slot local
__global__ void p2p_ag_kernel(PeerTable t, int world, long n16_loc, long half_bytes, u32x4* __restrict__ out,
                              const uint32_t* __restrict__ epoch) {
  const int h = ((epoch[0] - 2) >> 1) & 1;
  const long off = FLAG_BYTES + h * half_bytes;
  const long n = n16_loc * world;
  DTC_ASSERT(16 * n <= half_bytes && world >= 1);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    out[i] = ((const u32x4*)(t.base[(int)(i / n16_loc)] + off))[i];
}

// ---------------------------------------------------------------- pipeline stage messages (pp_comm: p2p)
// A point-to-point message between neighbouring pipeline stages, built from the signalling pattern of
// the barrier above and PULLED by its receiver:
//
//   sender    payload -> a slot of its OWN buffer (pp_stage_kernel, or the producer wrote it there)
//             kernel boundary
//             pp_signal_kernel: __threadfence_system, release store of the step epoch into flag word
//             `flag_idx` of the RECEIVER's buffer (system scope).  A send never waits.
//   receiver  pp_wait_kernel: spins on its own flag word (system-scope acquire) until it is >= the step
//             epoch; bounded like the barrier (error word 3000 + flag_idx, then proceeds)
//             kernel boundary
//             pp_pull_kernel: loads the sender's slot over the mapped pointer into the destination
//             (16-byte pieces, any element type; optionally also the fp32 image of a bf16 message)
//
// No payload is ever stored remotely.  The step epoch is a device counter bumped once per step
// (dtc_epoch_inc), so eager steps and graph replays advance it alike; each (direction, kind, microbatch)
// has its own slot and flag word (parallel/p2p.py P2PPipe), written once per step.
__global__ void pp_stage_kernel(const u32x4* __restrict__ x, u32x4* __restrict__ slot, long n16, long slot_off,
                                long buf_bytes) {
  DTC_ASSERT(slot_off >= 0 && slot_off % 16 == 0 && slot_off + 16 * n16 <= buf_bytes);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x) slot[i] = x[i];
}

__global__ void pp_signal_kernel(uint32_t* __restrict__ peer_flags, int flag_idx, const uint32_t* __restrict__ epoch) {
  DTC_ASSERT(flag_idx >= 0 && flag_idx < FLAG_BYTES / 4);
  if (threadIdx.x == 0) {
    __threadfence_system();  // the slot's content (earlier kernels of this stream) before the signal
    __hip_atomic_store(peer_flags + flag_idx, epoch[0], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ void pp_wait_kernel(const uint32_t* __restrict__ flags, int flag_idx, const uint32_t* __restrict__ epoch,
                               int* __restrict__ err) {
  DTC_ASSERT(flag_idx >= 0 && flag_idx < FLAG_BYTES / 4);
  if (threadIdx.x == 0) {
    const uint32_t e = epoch[0];
    const uint64_t t0 = wall_clock();
    while (__hip_atomic_load(flags + flag_idx, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < e) {
      __builtin_amdgcn_s_sleep(2);
      if (wall_clock() - t0 > 1000000000ull) {  // ~10 s at 100 MHz
        atomicExch(err, 3000 + flag_idx);
        break;
      }
    }
  }
  __syncthreads();
}

// out[i] = slot[i] (16-byte pieces); F32: the piece holds 8 bf16 values, whose exact fp32 images
// (bits << 16) also go to out_f32[8 i .. 8 i + 7]
template <bool F32>
__global__ void pp_pull_kernel(const u32x4* __restrict__ slot, u32x4* __restrict__ out, u32x4* __restrict__ out_f32,
                               long n16, long slot_off, long buf_bytes) {
  DTC_ASSERT(slot_off >= 0 && slot_off % 16 == 0 && slot_off + 16 * n16 <= buf_bytes);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x) {
    const u32x4 v = slot[i];
    out[i] = v;
    if constexpr (F32) {
      out_f32[2 * i] = u32x4{v[0] << 16, v[0] & 0xffff0000u, v[1] << 16, v[1] & 0xffff0000u};
      out_f32[2 * i + 1] = u32x4{v[2] << 16, v[2] & 0xffff0000u, v[3] << 16, v[3] & 0xffff0000u};
    }
  }
}

// ---------------------------------------------------------------- DP gradient buckets (dp_comm: p2p)
// The two-shot all-reduce above, for a bucket of the flat fp32 gradient buffer, in place:
//
//   pack     grads -> own half h in 16-byte pieces; with a bf16 payload rounded (f2bf) while copying, 8
//            elements per piece, the last piece zero-padded when n % 8 == 4
//   barrier
//   reduce   rank r sums pieces [r chunk, (r + 1) chunk) of every rank's half, in rank order, into its own
//            half (chunk = ceil(pieces / W): trailing ranks may own a short or an empty slice).
//            fp32: s = x[0]; s += x[p].   bf16: a = 0; a += float(x[p]); one f2bf (shard_sum_bf16_kernel)
//   barrier
//   gather   grads[piece i] = the piece of slice owner i / chunk; bf16 widened exactly (bits << 16);
//            nothing is written at or behind grads + n
//
// These kernels run UNDER the backward GEMMs, so their grid is capped by the caller (max_blocks blocks of
// 256 threads) and each thread keeps several 16-byte loads in flight instead: DP_U pieces in the copies,
// all W peers' loads of DP_RU pieces before the first add in the reduction.
constexpr int DP_U = 4;
constexpr int DP_RU = 2;

template <bool BF16>
__global__ void __launch_bounds__(256) dp_pack_kernel(const float* __restrict__ g, PeerTable t, int rank, long n,
                                                      long pieces, long half_bytes,
                                                      const uint32_t* __restrict__ epoch) {
  const int h = (epoch[0] >> 1) & 1;
  DTC_ASSERT(n > 0 && n % 4 == 0 && pieces == (BF16 ? (n + 7) / 8 : n / 4) && 16 * pieces <= half_bytes &&
             rank >= 0 && rank < P2P_MAX);
  unsigned char* dst = t.base[rank] + FLAG_BYTES + h * half_bytes;
  const f32x4* g4 = (const f32x4*)g;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x; i0 < pieces; i0 += DP_U * stride) {
    if constexpr (BF16) {
      f32x4 a[DP_U], b[DP_U];
#pragma unroll
      for (int u = 0; u < DP_U; ++u) {
        const long i = i0 + u * stride;
        a[u] = b[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i < pieces) {
          DTC_ASSERT(8 * i + 4 <= n);
          a[u] = g4[2 * i];
          if (8 * i + 4 < n) b[u] = g4[2 * i + 1];  // else: the zero pad of the last piece
        }
      }
#pragma unroll
      for (int u = 0; u < DP_U; ++u) {
        const long i = i0 + u * stride;
        if (i < pieces) {
          bf16x8 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) { o[e] = f2bf(a[u][e]); o[e + 4] = f2bf(b[u][e]); }
          ((bf16x8*)dst)[i] = o;
        }
      }
    } else {
      f32x4 a[DP_U];
#pragma unroll
      for (int u = 0; u < DP_U; ++u) {
        const long i = i0 + u * stride;
        if (i < pieces) a[u] = g4[i];
      }
#pragma unroll
      for (int u = 0; u < DP_U; ++u) {
        const long i = i0 + u * stride;
        if (i < pieces) ((f32x4*)dst)[i] = a[u];
      }
    }
  }
}

template <bool BF16>
__global__ void __launch_bounds__(256) dp_reduce_kernel(PeerTable t, int rank, int world, long pieces, long half_bytes,
                                                        const uint32_t* __restrict__ epoch) {
  using V = typename std::conditional<BF16, bf16x8, f32x4>::type;
  const int h = ((epoch[0] - 1) >> 1) & 1;  // one barrier has passed since the pack
  const long chunk = (pieces + world - 1) / world;
  const long lo = min(pieces, rank * chunk), hi = min(pieces, lo + chunk);
  const long off = FLAG_BYTES + h * half_bytes;
  DTC_ASSERT(world >= 1 && world <= P2P_MAX && rank >= 0 && rank < world && pieces > 0 && 16 * pieces <= half_bytes &&
             chunk * world >= pieces && lo <= hi && hi <= pieces);
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i0 = lo + (long)blockIdx.x * blockDim.x + threadIdx.x; i0 < hi; i0 += DP_RU * stride) {
    V v[DP_RU][P2P_MAX];
#pragma unroll
    for (int u = 0; u < DP_RU; ++u) {
      const long i = i0 + u * stride;
      if (i < hi) {
#pragma unroll
        for (int p = 0; p < P2P_MAX; ++p)
          if (p < world) v[u][p] = ((const V*)(t.base[p] + off))[i];
      }
    }
#pragma unroll
    for (int u = 0; u < DP_RU; ++u) {
      const long i = i0 + u * stride;
      if (i < hi) {
        if constexpr (BF16) {
          float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int p = 0; p < P2P_MAX; ++p)
            if (p < world) add8(a, v[u][p]);
          bf16x8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = f2bf(a[e]);
          ((bf16x8*)(t.base[rank] + off))[i] = o;
        } else {
          f32x4 s = v[u][0];
#pragma unroll
          for (int p = 1; p < P2P_MAX; ++p)
            if (p < world) s += v[u][p];
          ((f32x4*)(t.base[rank] + off))[i] = s;
        }
      }
    }
  }
}

template <bool BF16>
__global__ void __launch_bounds__(256) dp_gather_kernel(PeerTable t, int world, long n, long pieces, long half_bytes,
                                                        float* __restrict__ out, const uint32_t* __restrict__ epoch) {
  const int h = ((epoch[0] - 2) >> 1) & 1;
  const long chunk = (pieces + world - 1) / world;
  const long off = FLAG_BYTES + h * half_bytes;
  DTC_ASSERT(world >= 1 && world <= P2P_MAX && n > 0 && n % 4 == 0 && pieces == (BF16 ? (n + 7) / 8 : n / 4) &&
             16 * pieces <= half_bytes);
  u32x4* out4 = (u32x4*)out;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x; i0 < pieces; i0 += DP_U * stride) {
    u32x4 v[DP_U];
#pragma unroll
    for (int u = 0; u < DP_U; ++u) {
      const long i = i0 + u * stride;
      if (i < pieces) {
        const int q = (int)(i / chunk);
        DTC_ASSERT(q >= 0 && q < world);
        v[u] = ((const u32x4*)(t.base[q] + off))[i];
      }
    }
#pragma unroll
    for (int u = 0; u < DP_U; ++u) {
      const long i = i0 + u * stride;
      if (i < pieces) {
        if constexpr (BF16) {
          DTC_ASSERT(8 * i + 4 <= n);
          out4[2 * i] = u32x4{v[u][0] << 16, v[u][0] & 0xffff0000u, v[u][1] << 16, v[u][1] & 0xffff0000u};
          if (8 * i + 4 < n)  // the last piece of n % 8 == 4 holds 4 elements: never write past out + n
            out4[2 * i + 1] = u32x4{v[u][2] << 16, v[u][2] & 0xffff0000u, v[u][3] << 16, v[u][3] & 0xffff0000u};
        } else {
          out4[i] = v[u];
        }
      }
    }
  }
}

// ---------------------------------------------------------------- ZeRO-1 over the DP buckets (zero_comm: p2p)
// The bucket all-reduce above cut in the middle: the sharded AdamW sits on the reduced slice, and the gather moves
// the updated parameters instead of the gradients.
//
//   reduce-scatter   pack (dp_pack_kernel, as is) -> barrier (+2) -> dp_reduce_shard_kernel: the loads and the sums
//                    of dp_reduce_kernel, but the result goes as fp32 straight into grads[own slice] (bf16 widened
//                    exactly), so those elements hold bit for bit what dtc_dp_allreduce would have left there, and
//                    the slice's sum of squares goes to one partial per block (fixed order: per thread in loop
//                    order, the wave by xor shuffles, the 4 waves through LDS in wave order; no atomics)
//   parameter gather pack of the owned fp32 parameter slice, compact at the start of the half -> barrier (+2) ->
//                    dp_gather_params_kernel: every 4-float group of the bucket from its owner (own slice: local
//                    memory, not rewritten), written to params and, rounded like cast_kernel, to the bf16 mirror
//
// ONE barrier per call is enough.  A call only READS the peers' halves after its barrier (it writes local memory),
// the halves alternate per call and every call advances the epoch by 2.  Call k + 2 rewrites half h only after this
// rank passed call k + 1's barrier; a rank signals that barrier only after its call-k kernels have finished reading
// half h, because the barrier kernel follows them in stream order.  This needs every call of the object in ONE
// stream order on every rank, which is how parallel/p2p.py issues them (P2PGradReduce.on_comm: one comm stream,
// forked from and joined to the step's stream by events; or the step's stream itself).  The two-barrier calls of
// the object (dtc_dp_allreduce, the two-shot sum) and the one-barrier ones mix freely under the same argument: a
// half is written remotely by nobody, and locally only before the call's first barrier or, in the two-shot
// reduction, between its two barriers by its owner alone.
template <bool BF16>
__global__ void __launch_bounds__(256) dp_reduce_shard_kernel(PeerTable t, int rank, int world, long n, long pieces,
                                                              long half_bytes, float* __restrict__ grads,
                                                              float* __restrict__ part,
                                                              const uint32_t* __restrict__ epoch) {
  using V = typename std::conditional<BF16, bf16x8, f32x4>::type;
  const int h = ((epoch[0] - 2) >> 1) & 1;  // the call's one barrier (+2) has passed since the pack
  const long chunk = (pieces + world - 1) / world;
  const long lo = min(pieces, rank * chunk), hi = min(pieces, lo + chunk);
  const long off = FLAG_BYTES + h * half_bytes;
  DTC_ASSERT(world >= 1 && world <= P2P_MAX && rank >= 0 && rank < world && n > 0 && n % 4 == 0 &&
             pieces == (BF16 ? (n + 7) / 8 : n / 4) && 16 * pieces <= half_bytes && chunk * world >= pieces &&
             lo <= hi && hi <= pieces);
  f32x4* g4 = (f32x4*)grads;
  float sq = 0.f;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i0 = lo + (long)blockIdx.x * blockDim.x + threadIdx.x; i0 < hi; i0 += DP_RU * stride) {
    V v[DP_RU][P2P_MAX];
#pragma unroll
    for (int u = 0; u < DP_RU; ++u) {
      const long i = i0 + u * stride;
      if (i < hi) {
#pragma unroll
        for (int p = 0; p < P2P_MAX; ++p)
          if (p < world) v[u][p] = ((const V*)(t.base[p] + off))[i];
      }
    }
#pragma unroll
    for (int u = 0; u < DP_RU; ++u) {
      const long i = i0 + u * stride;
      if (i < hi) {
        if constexpr (BF16) {
          float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int p = 0; p < P2P_MAX; ++p)
            if (p < world) add8(a, v[u][p]);
#pragma unroll
          for (int e = 0; e < 8; ++e) a[e] = (float)f2bf(a[e]);  // one rounding; the widening is exact
          DTC_ASSERT(8 * i + 4 <= n);
          g4[2 * i] = f32x4{a[0], a[1], a[2], a[3]};
#pragma unroll
          for (int e = 0; e < 4; ++e) sq = fmaf(a[e], a[e], sq);
          if (8 * i + 4 < n) {  // the last piece of n % 8 == 4 holds 4 elements: never write past grads + n
            g4[2 * i + 1] = f32x4{a[4], a[5], a[6], a[7]};
#pragma unroll
            for (int e = 4; e < 8; ++e) sq = fmaf(a[e], a[e], sq);
          }
        } else {
          f32x4 s = v[u][0];
#pragma unroll
          for (int p = 1; p < P2P_MAX; ++p)
            if (p < world) s += v[u][p];
          DTC_ASSERT(4 * i + 4 <= n);
          g4[i] = s;
#pragma unroll
          for (int e = 0; e < 4; ++e) sq = fmaf(s[e], s[e], sq);
        }
      }
    }
  }
  // one partial per block, every block (an empty slice: zeros)
  __shared__ float wsum[4];
  sq = warp_sum(sq);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// 4-float groups [q_lo, q_hi) of params -> the start of own half h (the slice this rank owns and has just updated)
__global__ void __launch_bounds__(256) dp_pack_params_kernel(const float* __restrict__ params, PeerTable t, int rank,
                                                             long q_lo, long q_hi, long half_bytes,
                                                             const uint32_t* __restrict__ epoch) {
  const int h = (epoch[0] >> 1) & 1;
  DTC_ASSERT(rank >= 0 && rank < P2P_MAX && 0 <= q_lo && q_lo <= q_hi && 16 * (q_hi - q_lo) <= half_bytes);
  f32x4* dst = (f32x4*)(t.base[rank] + FLAG_BYTES + h * half_bytes);
  const f32x4* p4 = (const f32x4*)params + q_lo;
  const long nq = q_hi - q_lo;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x; i0 < nq; i0 += DP_U * stride) {
    f32x4 a[DP_U];
#pragma unroll
    for (int u = 0; u < DP_U; ++u) {
      const long i = i0 + u * stride;
      if (i < nq) a[u] = p4[i];
    }
#pragma unroll
    for (int u = 0; u < DP_U; ++u) {
      const long i = i0 + u * stride;
      if (i < nq) dst[i] = a[u];
    }
  }
}

// params[4-float group i] = the group of its owner (piece i / qpp belongs to rank piece / chunk; that rank's slice
// sits compact at the start of its half); own groups are read from params.  mirror[4 i .. 4 i + 3] = bf16 of the
// same values for 4 i < n_mirror.  Nothing is written at or behind params + n or mirror + n_mirror.
__global__ void __launch_bounds__(256) dp_gather_params_kernel(PeerTable t, int rank, int world, long n, long pieces,
                                                               int qpp, long half_bytes, float* __restrict__ params,
                                                               bf16* __restrict__ mirror, long n_mirror,
                                                               const uint32_t* __restrict__ epoch) {
  const int h = ((epoch[0] - 2) >> 1) & 1;
  const long chunk = (pieces + world - 1) / world;
  const long off = FLAG_BYTES + h * half_bytes;
  const long nq = n / 4;
  DTC_ASSERT(world >= 1 && world <= P2P_MAX && rank >= 0 && rank < world && n > 0 && n % 4 == 0 &&
             (qpp == 1 || qpp == 2) && pieces == (nq + qpp - 1) / qpp && n_mirror >= 0 && n_mirror <= n &&
             n_mirror % 4 == 0 && 16 * min(nq, chunk * qpp) <= half_bytes);
  f32x4* p4 = (f32x4*)params;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i0 = (long)blockIdx.x * blockDim.x + threadIdx.x; i0 < nq; i0 += DP_U * stride) {
    f32x4 v[DP_U];
    bool own[DP_U];
#pragma unroll
    for (int u = 0; u < DP_U; ++u) {
      const long i = i0 + u * stride;
      own[u] = true;
      if (i < nq) {
        const int q = (int)((i / qpp) / chunk);
        DTC_ASSERT(q >= 0 && q < world && i >= q * chunk * qpp && 16 * (i - q * chunk * qpp + 1) <= half_bytes);
        own[u] = q == rank;
        v[u] = own[u] ? p4[i] : ((const f32x4*)(t.base[q] + off))[i - q * chunk * qpp];
      }
    }
#pragma unroll
    for (int u = 0; u < DP_U; ++u) {
      const long i = i0 + u * stride;
      if (i < nq) {
        if (!own[u]) p4[i] = v[u];
        if (4 * i < n_mirror)
          *(bf16x4*)(mirror + 4 * i) = bf16x4{f2bf(v[u][0]), f2bf(v[u][1]), f2bf(v[u][2]), f2bf(v[u][3])};
      }
    }
  }
}

// ---------------------------------------------------------------- intra-device stream flags
// Cross-stream dependencies between two separately captured hipGraphs (main / side) on the SAME
// device: a producer stream bumps flags[k] to its replay epoch (agent-scope release, after all of
// its prior kernels completed in queue order); the consumer spins until flags[k] >= its own
// epoch (agent-scope acquire).  Each graph bumps its epoch once per replay, so the two stay in
// lock step without host involvement.  Spins are bounded (~10 s -> error word, then proceed).
__global__ void epoch_inc_kernel(uint32_t* __restrict__ epoch) {
  if (threadIdx.x == 0) epoch[0] += 1;
}

__global__ void flag_set_kernel(uint32_t* __restrict__ flags, int k, const uint32_t* __restrict__ epoch) {
  if (threadIdx.x == 0) {
    __threadfence();
    __hip_atomic_store(flags + k, epoch[0], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void flag_wait_kernel(const uint32_t* __restrict__ flags, int k, const uint32_t* __restrict__ epoch,
                                 int* __restrict__ err) {
  if (threadIdx.x == 0) {
    const uint32_t e = epoch[0];
    const uint64_t t0 = wall_clock();
    while (__hip_atomic_load(flags + k, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < e) {
      __builtin_amdgcn_s_sleep(1);
      if (wall_clock() - t0 > 1000000000ull) {
        atomicExch(err, 2000 + k);
        break;
      }
    }
  }
  __syncthreads();
}

// CU-occupancy probe (benchmarks/cu_steal_proxy.py): `blocks` workgroups, each requesting (nearly) a whole CU's
// LDS so no other LDS-using workgroup fits next to it, idle for `ticks` of the 100 MHz wall clock -- a stand-in
// for the CUs an RCCL collective holds while the step's kernels run on the rest.  Bounded: every wave exits.
__global__ void cu_hog_kernel(uint64_t ticks, int* __restrict__ sink) {
  extern __shared__ int hog_lds[];
  // sink[1] (host-mapped): workgroups resident so far -- the host starts timing once all are
  if (threadIdx.x == 0) __hip_atomic_fetch_add(sink + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  const uint64_t t0 = wall_clock();
  while (wall_clock() - t0 < ticks) __builtin_amdgcn_s_sleep(16);
  hog_lds[threadIdx.x] = (int)threadIdx.x;
  __syncthreads();
  if (threadIdx.x == 0 && hog_lds[1] == 12345) sink[0] = 1;  // never true: keeps the LDS allocation live
}

}  // namespace

extern "C" {

int dtc_epoch_inc(uint32_t* epoch, hipStream_t st) {
  hipLaunchKernelGGL(epoch_inc_kernel, dim3(1), dim3(64), 0, st, epoch);
  DTC_CHECK_LAUNCH();
  return 0;
}

int dtc_flag_set(uint32_t* flags, int k, const uint32_t* epoch, hipStream_t st) {
  hipLaunchKernelGGL(flag_set_kernel, dim3(1), dim3(64), 0, st, flags, k, epoch);
  DTC_CHECK_LAUNCH();
  return 0;
}

int dtc_flag_wait(const uint32_t* flags, int k, const uint32_t* epoch, int* err, hipStream_t st) {
  hipLaunchKernelGGL(flag_wait_kernel, dim3(1), dim3(64), 0, st, flags, k, epoch, err);
  DTC_CHECK_LAUNCH();
  return 0;
}

long dtc_p2p_flag_bytes() { return FLAG_BYTES; }

// uncached device buffer (flags + 2 data halves) and its IPC handle (64 bytes)
int dtc_p2p_alloc(long bytes, void** ptr, char* handle) {
  hipError_t e = hipExtMallocWithFlags(ptr, (size_t)bytes, hipDeviceMallocUncached);
  if (e != hipSuccess) return (int)e;
  e = hipMemset(*ptr, 0, FLAG_BYTES);
  if (e != hipSuccess) return (int)e;
  hipIpcMemHandle_t h;
  e = hipIpcGetMemHandle(&h, *ptr);
  if (e != hipSuccess) return (int)e;
  static_assert(sizeof(hipIpcMemHandle_t) <= 64, "handle size");
  memcpy(handle, &h, sizeof(h));
  return 0;
}

int dtc_p2p_open(const char* handle, void** ptr) {
  hipIpcMemHandle_t h;
  memcpy(&h, handle, sizeof(h));
  return (int)hipIpcOpenMemHandle(ptr, h, hipIpcMemLazyEnablePeerAccess);
}

int dtc_p2p_close(void* ptr) { return (int)hipIpcCloseMemHandle(ptr); }

// Topology checks at P2P init (parallel/p2p.py): the PCI bus id identifies a GPU across processes
// (device ordinals depend on each process's visible set); can-access-peer says whether a kernel on
// `dev` can load `peer`'s memory directly (xGMI).
int dtc_device_pci_bus_id(int dev, char* buf, int len) { return (int)hipDeviceGetPCIBusId(buf, len, dev); }
int dtc_device_count(int* n) { return (int)hipGetDeviceCount(n); }
int dtc_can_access_peer(int dev, int peer, int* ok) { return (int)hipDeviceCanAccessPeer(ok, dev, peer); }
int dtc_p2p_free(void* ptr) { return (int)hipFree(ptr); }
// Node count of a captured (not yet instantiated) hipGraph: parallel/program.py drops segments that
// captured nothing (e.g. between a collective and its wait) instead of replaying empty graphs.
int dtc_graph_num_nodes(void* graph, size_t* n) { return (int)hipGraphGetNodes((hipGraph_t)graph, nullptr, n); }

// out = sum over ranks of x (fp32, n % 4 == 0, n*4 <= half_bytes).  x and out may alias.
// mode: 0 auto, 1 two-shot, 2 one-shot.  Per link, one-shot moves n bytes (each rank reads every peer
// once over that peer's link) and two-shot 2n/W, for one barrier fewer: at W = 2 the bytes are equal
// and one-shot always wins; at W = 4 / 8 it wins up to ~1 MB / 512 KB (a barrier round trip is a few
// us, a link ~150 GB/s).  Measured with 2 ranks on one device (benchmarks/p2p_bench.py): one-shot
// 6.5 / 7.5 / 11.9 / 16.9 us vs two-shot 11.2 (512 KB) / 12.3 / 18.5 / 22.8 us at 64 KB / 1 / 4 / 8 MB.
constexpr long P2P_ONESHOT_BYTES = 512 * 1024;
inline bool oneshot_auto(long bytes, int world) {
  return world <= 2 || bytes <= P2P_ONESHOT_BYTES * (world <= 4 ? 2 : 1);
}
int dtc_p2p_allreduce(const float* x, float* out, long n, void* const* bases, int rank, int world, long half_bytes,
                      uint32_t* epoch, int* err, int mode, hipStream_t st) {
  if (world < 1 || world > P2P_MAX || n % 4 || n * 4 > half_bytes) return 4001;
  PeerTable t;
  for (int p = 0; p < P2P_MAX; ++p) t.base[p] = (unsigned char*)(p < world ? bases[p] : nullptr);
  const long n4 = n / 4;
  const int blocks = (int)std::min(1024L, std::max(1L, (n4 + 255) / 256));
  const bool one = mode == 2 || (mode == 0 && oneshot_auto(n * 4, world));
  hipLaunchKernelGGL(p2p_stage_kernel, dim3(blocks), dim3(256), 0, st, (const f32x4*)x, t, rank, n4, half_bytes, epoch);
  DTC_CHECK_LAUNCH();
  if (one) {
    hipLaunchKernelGGL(p2p_barrier_kernel, dim3(1), dim3(64), 0, st, t, rank, world, epoch, err, 2);
    DTC_CHECK_LAUNCH();
    hipLaunchKernelGGL(p2p_oneshot_kernel, dim3(blocks), dim3(256), 0, st, t, world, n4, half_bytes, (f32x4*)out,
                       epoch);
    DTC_CHECK_LAUNCH();
    return 0;
  }
  hipLaunchKernelGGL(p2p_barrier_kernel, dim3(1), dim3(64), 0, st, t, rank, world, epoch, err, 1);
  DTC_CHECK_LAUNCH();
  const int rs_blocks = (int)std::min(1024L, std::max(1L, (n4 / world + 255) / 256));
  hipLaunchKernelGGL(p2p_reduce_scatter_kernel, dim3(rs_blocks), dim3(256), 0, st, t, rank, world, n4, half_bytes,
                     epoch);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(p2p_barrier_kernel, dim3(1), dim3(64), 0, st, t, rank, world, epoch, err, 1);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(p2p_all_gather_kernel, dim3(blocks), dim3(256), 0, st, t, world, n4, half_bytes, (f32x4*)out,
                     epoch);
  DTC_CHECK_LAUNCH();
  return 0;
}

// out (fp32) = resid + bias + sum over ranks of x (bf16, n % 8 == 0, n * 2 <= half_bytes); resid / bias
// optional (null), bias indexed by column (ncols % 8 == 0).  mode as dtc_p2p_allreduce; x may not alias out.
// x == nullptr: the partial is already in this rank's buffer half of the call (the row-parallel GEMM wrote
// it there, parallel/p2p.py staged_out): no stage launch -- barrier + one-shot (2 launches) or barrier +
// reduce-scatter + barrier + all-gather (4).
int dtc_p2p_allreduce_bf16(const bf16* x, float* out, long n, void* const* bases, int rank, int world, long half_bytes,
                           uint32_t* epoch, int* err, int mode, const float* resid, const float* bias, int ncols,
                           hipStream_t st) {
  if (world < 1 || world > P2P_MAX || n % 8 || n * 2 > half_bytes || (bias && (ncols <= 0 || ncols % 8))) return 4001;
  PeerTable t;
  for (int p = 0; p < P2P_MAX; ++p) t.base[p] = (unsigned char*)(p < world ? bases[p] : nullptr);
  const long n8 = n / 8;
  const int blocks = (int)std::min(1024L, std::max(1L, (n8 + 255) / 256));
  const bool one = mode == 2 || (mode == 0 && oneshot_auto(n * 2, world));
  if (x) {
    hipLaunchKernelGGL(p2p_stage_bf16_kernel, dim3(blocks), dim3(256), 0, st, (const bf16x8*)x, t, rank, n8,
                       half_bytes, epoch);
    DTC_CHECK_LAUNCH();
  }
  if (one) {
    hipLaunchKernelGGL(p2p_barrier_kernel, dim3(1), dim3(64), 0, st, t, rank, world, epoch, err, 2);
    DTC_CHECK_LAUNCH();
    hipLaunchKernelGGL(p2p_oneshot_bf16_kernel, dim3(blocks), dim3(256), 0, st, t, world, n8, half_bytes, out, resid,
                       bias, ncols, epoch);
    DTC_CHECK_LAUNCH();
    return 0;
  }
  hipLaunchKernelGGL(p2p_barrier_kernel, dim3(1), dim3(64), 0, st, t, rank, world, epoch, err, 1);
  DTC_CHECK_LAUNCH();
  const int rs_blocks = (int)std::min(1024L, std::max(1L, (n8 / world + 255) / 256));
  hipLaunchKernelGGL(p2p_reduce_scatter_bf16_kernel, dim3(rs_blocks), dim3(256), 0, st, t, rank, world, n8, half_bytes,
                     epoch);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(p2p_barrier_kernel, dim3(1), dim3(64), 0, st, t, rank, world, epoch, err, 1);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(p2p_all_gather_bf16_kernel, dim3(blocks), dim3(256), 0, st, t, world, n8, half_bytes, out, resid,
                     bias, ncols, epoch);
  DTC_CHECK_LAUNCH();
  return 0;
}

// ---- sequence-parallel collectives (one barrier each, epoch + 2 per call like the one-shot all-reduce)
// reduce-scatter of a [W * n_loc] partial (bf16 if bf16 else fp32) into this rank's n_loc fp32 elements:
// out = resid + bias + sum_ranks partial[rank * n_loc .. +n_loc].  x == nullptr: the producer wrote the
// partial into this call's buffer half (staged_out).  n_loc % 8 == 0; bias by column (ncols % 8 == 0,
// n_loc % ncols == 0: whole rows per rank).
int dtc_p2p_reduce_scatter(const void* x, int bf16, float* out, long n_loc, void* const* bases, int rank, int world,
                           long half_bytes, uint32_t* epoch, int* err, const float* resid, const float* bias,
                           int ncols, hipStream_t st) {
  const long esz = bf16 ? 2 : 4;
  if (world < 1 || world > P2P_MAX || n_loc % 8 || n_loc * world * esz > half_bytes ||
      (bias && (ncols <= 0 || ncols % 8 || n_loc % ncols)))
    return 4001;
  PeerTable t;
  for (int p = 0; p < P2P_MAX; ++p) t.base[p] = (unsigned char*)(p < world ? bases[p] : nullptr);
  if (x) {
    const long n16 = n_loc * world * esz / 16;
    const int sb = (int)std::min(1024L, std::max(1L, (n16 + 255) / 256));
    hipLaunchKernelGGL(p2p_stage16_kernel, dim3(sb), dim3(256), 0, st, (const u32x4*)x, t, rank, 0L, n16, half_bytes,
                       epoch);
    DTC_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(p2p_barrier_kernel, dim3(1), dim3(64), 0, st, t, rank, world, epoch, err, 2);
  DTC_CHECK_LAUNCH();
  const long n8 = n_loc / 8;
  const int blocks = (int)std::min(1024L, std::max(1L, (n8 + 255) / 256));
  if (bf16)
    hipLaunchKernelGGL(p2p_rs_kernel<true>, dim3(blocks), dim3(256), 0, st, t, rank, world, n8, half_bytes, out, resid,
                       bias, ncols, epoch);
  else
    hipLaunchKernelGGL(p2p_rs_kernel<false>, dim3(blocks), dim3(256), 0, st, t, rank, world, n8, half_bytes, out,
                       resid, bias, ncols, epoch);
  DTC_CHECK_LAUNCH();
  return 0;
}

// all-gather of this rank's loc_bytes (x, a multiple of 16) into out [W * loc_bytes], rank-major.
// x == nullptr: the producer already wrote the slot (staged_out at offset rank * loc_bytes).
int dtc_p2p_all_gather(const void* x, void* out, long loc_bytes, void* const* bases, int rank, int world,
                       long half_bytes, uint32_t* epoch, int* err, hipStream_t st) {
  if (world < 1 || world > P2P_MAX || loc_bytes % 16 || loc_bytes * world > half_bytes) return 4001;
  PeerTable t;
  for (int p = 0; p < P2P_MAX; ++p) t.base[p] = (unsigned char*)(p < world ? bases[p] : nullptr);
  const long n16 = loc_bytes / 16;
  if (x) {
    const int sb = (int)std::min(1024L, std::max(1L, (n16 + 255) / 256));
    hipLaunchKernelGGL(p2p_stage16_kernel, dim3(sb), dim3(256), 0, st, (const u32x4*)x, t, rank, rank * n16, n16,
                       half_bytes, epoch);
    DTC_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(p2p_barrier_kernel, dim3(1), dim3(64), 0, st, t, rank, world, epoch, err, 2);
  DTC_CHECK_LAUNCH();
  const int blocks = (int)std::min(1024L, std::max(1L, (n16 * world + 255) / 256));
  hipLaunchKernelGGL(p2p_ag_kernel, dim3(blocks), dim3(256), 0, st, t, world, n16, half_bytes, (u32x4*)out, epoch);
  DTC_CHECK_LAUNCH();
  return 0;
}

// ---- pipeline stage messages (kernels above; slot table and flag indices: parallel/p2p.py P2PPipe)
inline bool pp_args_ok(long n, long slot_off, long buf_bytes, int flag_idx) {
  return n > 0 && n % 16 == 0 && slot_off >= 0 && slot_off % 16 == 0 && slot_off <= buf_bytes &&
         n <= buf_bytes - slot_off && flag_idx >= 0 && flag_idx < FLAG_BYTES / 4;
}

// Send n bytes (a multiple of 16): copy x into this rank's slot at payload offset slot_off of its own buffer
// (own_base; buf_bytes of payload behind the flag area), then store the step epoch into flag word flag_idx
// of the receiver's buffer (peer_base).  x == nullptr: the producer already wrote the slot.  Never waits.
int dtc_pp_send(const void* x, long n, void* own_base, long slot_off, long buf_bytes, void* peer_base, int flag_idx,
                const uint32_t* epoch, hipStream_t st) {
  if (!own_base || !peer_base || !epoch || !pp_args_ok(n, slot_off, buf_bytes, flag_idx) || ((uintptr_t)x & 15))
    return 4001;
  if (x) {
    const long n16 = n / 16;
    const int blocks = (int)std::min(1024L, std::max(1L, (n16 + 255) / 256));
    hipLaunchKernelGGL(pp_stage_kernel, dim3(blocks), dim3(256), 0, st, (const u32x4*)x,
                       (u32x4*)((unsigned char*)own_base + FLAG_BYTES + slot_off), n16, slot_off, buf_bytes);
    DTC_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(pp_signal_kernel, dim3(1), dim3(64), 0, st, (uint32_t*)peer_base, flag_idx, epoch);
  DTC_CHECK_LAUNCH();
  return 0;
}

// Receive n bytes: wait until this rank's flag word flag_idx (own_base) reaches the step epoch, then copy the
// sender's slot (peer_base, payload offset slot_off, buf_bytes of payload in the SENDER's buffer) into out.
// out_f32 (optional): the message is bf16 and its fp32 image (2 n bytes) is written in the same pass.
int dtc_pp_recv(void* out, void* out_f32, long n, const void* peer_base, long slot_off, long buf_bytes,
                const void* own_base, int flag_idx, const uint32_t* epoch, int* err, hipStream_t st) {
  if (!out || !own_base || !peer_base || !epoch || !err || !pp_args_ok(n, slot_off, buf_bytes, flag_idx) ||
      ((uintptr_t)out & 15) || ((uintptr_t)out_f32 & 15))
    return 4001;
  hipLaunchKernelGGL(pp_wait_kernel, dim3(1), dim3(64), 0, st, (const uint32_t*)own_base, flag_idx, epoch, err);
  DTC_CHECK_LAUNCH();
  const long n16 = n / 16;
  const int blocks = (int)std::min(1024L, std::max(1L, (n16 + 255) / 256));
  const u32x4* slot = (const u32x4*)((const unsigned char*)peer_base + FLAG_BYTES + slot_off);
  if (out_f32)
    hipLaunchKernelGGL(pp_pull_kernel<true>, dim3(blocks), dim3(256), 0, st, slot, (u32x4*)out, (u32x4*)out_f32, n16,
                       slot_off, buf_bytes);
  else
    hipLaunchKernelGGL(pp_pull_kernel<false>, dim3(blocks), dim3(256), 0, st, slot, (u32x4*)out, (u32x4*)nullptr, n16,
                       slot_off, buf_bytes);
  DTC_CHECK_LAUNCH();
  return 0;
}

// ---- DP gradient buckets (kernels above): grads[0:n] (fp32, 16-byte aligned, n a positive multiple of 4) =
// sum over ranks, in place.  bf16: the payload travels as bf16 (fp32 sums in rank order, one rounding of the
// reduced slice); ceil(n / 8) 16-byte pieces must fit the half, else n / 4.  Every grid is at most max_blocks
// blocks (1 .. 1024).  Epoch + 2 like every other call on the object.
int dtc_dp_allreduce(float* grads, long n, int bf16, void* const* bases, int rank, int world, long half_bytes,
                     uint32_t* epoch, int* err, int max_blocks, hipStream_t st) {
  if (!grads || !bases || !epoch || !err || world < 1 || world > P2P_MAX || rank < 0 || rank >= world || n <= 0 ||
      n % 4 || ((uintptr_t)grads & 15) || max_blocks < 1 || max_blocks > 1024 || half_bytes <= 0 || half_bytes % 16)
    return 4001;
  const long pieces = bf16 ? (n + 7) / 8 : n / 4;
  if (pieces > half_bytes / 16) return 4001;
  PeerTable t;
  for (int p = 0; p < P2P_MAX; ++p) t.base[p] = (unsigned char*)(p < world ? bases[p] : nullptr);
  const long chunk = (pieces + world - 1) / world;
  const int blocks = (int)std::min((long)max_blocks, std::max(1L, (pieces + 255) / 256));
  const int rs_blocks = (int)std::min((long)max_blocks, std::max(1L, (chunk + 255) / 256));
  if (bf16)
    hipLaunchKernelGGL(dp_pack_kernel<true>, dim3(blocks), dim3(256), 0, st, grads, t, rank, n, pieces, half_bytes,
                       epoch);
  else
    hipLaunchKernelGGL(dp_pack_kernel<false>, dim3(blocks), dim3(256), 0, st, grads, t, rank, n, pieces, half_bytes,
                       epoch);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(p2p_barrier_kernel, dim3(1), dim3(64), 0, st, t, rank, world, epoch, err, 1);
  DTC_CHECK_LAUNCH();
  if (bf16)
    hipLaunchKernelGGL(dp_reduce_kernel<true>, dim3(rs_blocks), dim3(256), 0, st, t, rank, world, pieces, half_bytes,
                       epoch);
  else
    hipLaunchKernelGGL(dp_reduce_kernel<false>, dim3(rs_blocks), dim3(256), 0, st, t, rank, world, pieces, half_bytes,
                       epoch);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(p2p_barrier_kernel, dim3(1), dim3(64), 0, st, t, rank, world, epoch, err, 1);
  DTC_CHECK_LAUNCH();
  if (bf16)
    hipLaunchKernelGGL(dp_gather_kernel<true>, dim3(blocks), dim3(256), 0, st, t, world, n, pieces, half_bytes, grads,
                       epoch);
  else
    hipLaunchKernelGGL(dp_gather_kernel<false>, dim3(blocks), dim3(256), 0, st, t, world, n, pieces, half_bytes, grads,
                       epoch);
  DTC_CHECK_LAUNCH();
  return 0;
}

// ---- ZeRO-1 over the DP buckets (kernels above).  Both calls: epoch + 2, one barrier.
// Blocks (= Σg² partial slots) of the reduce-scatter of an n-element bucket; the same on every rank.
int dtc_dp_rs_slots(long n, int bf16, int world, int max_blocks) {
  if (n <= 0 || n % 4 || world < 1 || world > P2P_MAX || max_blocks < 1 || max_blocks > 1024) return -1;
  const long pieces = bf16 ? (n + 7) / 8 : n / 4;
  const long chunk = (pieces + world - 1) / world;
  return (int)std::min((long)max_blocks, std::max(1L, (chunk + 255) / 256));
}

// grads[own slice] (fp32, in place) = sum over ranks of grads[own slice], where the own slice of the n-element
// bucket is pieces [min(pieces, rank chunk), min(pieces, (rank + 1) chunk)) of 4 fp32 / 8 bf16 elements, chunk =
// ceil(pieces / W): the values dtc_dp_allreduce leaves there.  Nothing else of grads is written.  part[0 : nslots]
// (nslots == dtc_dp_rs_slots(...)) = per-block partial sums of squares of the slice (zeros for an empty one).
int dtc_dp_reduce_scatter(float* grads, long n, int bf16, float* part, int nslots, void* const* bases, int rank,
                          int world, long half_bytes, uint32_t* epoch, int* err, int max_blocks, hipStream_t st) {
  if (!grads || !part || !bases || !epoch || !err || world < 1 || world > P2P_MAX || rank < 0 || rank >= world ||
      n <= 0 || n % 4 || ((uintptr_t)grads & 15) || ((uintptr_t)part & 3) || max_blocks < 1 || max_blocks > 1024 ||
      half_bytes <= 0 || half_bytes % 16)
    return 4001;
  const long pieces = bf16 ? (n + 7) / 8 : n / 4;
  if (pieces > half_bytes / 16 || nslots != dtc_dp_rs_slots(n, bf16, world, max_blocks)) return 4001;
  PeerTable t;
  for (int p = 0; p < P2P_MAX; ++p) t.base[p] = (unsigned char*)(p < world ? bases[p] : nullptr);
  const int blocks = (int)std::min((long)max_blocks, std::max(1L, (pieces + 255) / 256));
  if (bf16)
    hipLaunchKernelGGL(dp_pack_kernel<true>, dim3(blocks), dim3(256), 0, st, grads, t, rank, n, pieces, half_bytes,
                       epoch);
  else
    hipLaunchKernelGGL(dp_pack_kernel<false>, dim3(blocks), dim3(256), 0, st, grads, t, rank, n, pieces, half_bytes,
                       epoch);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(p2p_barrier_kernel, dim3(1), dim3(64), 0, st, t, rank, world, epoch, err, 2);
  DTC_CHECK_LAUNCH();
  if (bf16)
    hipLaunchKernelGGL(dp_reduce_shard_kernel<true>, dim3(nslots), dim3(256), 0, st, t, rank, world, n, pieces,
                       half_bytes, grads, part, epoch);
  else
    hipLaunchKernelGGL(dp_reduce_shard_kernel<false>, dim3(nslots), dim3(256), 0, st, t, rank, world, n, pieces,
                       half_bytes, grads, part, epoch);
  DTC_CHECK_LAUNCH();
  return 0;
}

// params[0:n] (fp32, one bucket) = every rank's owned slice of it (the ownership of dtc_dp_reduce_scatter with the
// same n, bf16 and world; bf16 only selects that plan, the parameters travel as fp32), own slice untouched;
// mirror[0:n_mirror] (bf16, optional, n_mirror <= n) = the rounded parameters, in the same pass.  Grids of at most
// max_blocks (1 .. 1024; the step's tail, nothing overlaps it: the caller passes 1024).
int dtc_dp_param_gather(float* params, bf16* mirror, long n, long n_mirror, int bf16_plan, void* const* bases,
                        int rank, int world, long half_bytes, uint32_t* epoch, int* err, int max_blocks,
                        hipStream_t st) {
  if (!params || !bases || !epoch || !err || world < 1 || world > P2P_MAX || rank < 0 || rank >= world || n <= 0 ||
      n % 4 || ((uintptr_t)params & 15) || ((uintptr_t)mirror & 7) || n_mirror < 0 || n_mirror > n || n_mirror % 4 ||
      (n_mirror > 0 && !mirror) || max_blocks < 1 || max_blocks > 1024 || half_bytes <= 0 || half_bytes % 16)
    return 4001;
  const int qpp = bf16_plan ? 2 : 1;
  const long nq = n / 4, pieces = (nq + qpp - 1) / qpp;
  const long chunk = (pieces + world - 1) / world;
  if (std::min(nq, chunk * qpp) > half_bytes / 16) return 4001;  // the largest slice (rank 0's) must fit the half
  const long q_lo = std::min(nq, rank * chunk * qpp), q_hi = std::min(nq, q_lo + chunk * qpp);
  PeerTable t;
  for (int p = 0; p < P2P_MAX; ++p) t.base[p] = (unsigned char*)(p < world ? bases[p] : nullptr);
  const int pk = (int)std::min((long)max_blocks, std::max(1L, (q_hi - q_lo + 255) / 256));
  hipLaunchKernelGGL(dp_pack_params_kernel, dim3(pk), dim3(256), 0, st, params, t, rank, q_lo, q_hi, half_bytes,
                     epoch);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(p2p_barrier_kernel, dim3(1), dim3(64), 0, st, t, rank, world, epoch, err, 2);
  DTC_CHECK_LAUNCH();
  const int blocks = (int)std::min((long)max_blocks, std::max(1L, (nq + 255) / 256));
  hipLaunchKernelGGL(dp_gather_params_kernel, dim3(blocks), dim3(256), 0, st, t, rank, world, n, pieces, qpp,
                     half_bytes, params, mirror, n_mirror, epoch);
  DTC_CHECK_LAUNCH();
  return 0;
}

int dtc_cu_hog(int blocks, long ticks, int lds_bytes, int* sink, hipStream_t st) {
  if (blocks <= 0) return 0;
  if (ticks <= 0 || ticks > 200000000L || lds_bytes < 1024) return 4001;  // at most 2 s
  hipError_t e = hipFuncSetAttribute((const void*)cu_hog_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(cu_hog_kernel, dim3(blocks), dim3(256), lds_bytes, st, (uint64_t)ticks, sink);
  DTC_CHECK_LAUNCH();
  return 0;
}

// A call with no payload (one barrier round, epoch + 2): keeps the number of calls per step even, so the
// buffer half of every call site -- which the host hands to a producer GEMM (staged_out) -- is the same
// on every replay of a captured step.
int dtc_p2p_barrier_round(void* const* bases, int rank, int world, uint32_t* epoch, int* err, hipStream_t st) {
  if (world < 1 || world > P2P_MAX) return 4001;
  PeerTable t;
  for (int p = 0; p < P2P_MAX; ++p) t.base[p] = (unsigned char*)(p < world ? bases[p] : nullptr);
  hipLaunchKernelGGL(p2p_barrier_kernel, dim3(1), dim3(64), 0, st, t, rank, world, epoch, err, 2);
  DTC_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"
