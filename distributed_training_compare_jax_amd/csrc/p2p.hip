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

// error word of a timed-out wait = base + the rank (barrier) or flag word (stream flags, stage messages) waited for
constexpr int ERR_BARRIER = 1000, ERR_FLAG = 2000, ERR_PP = 3000;

// The bounded spin of every wait here: until *flag >= e (acquire at SCOPE, s_sleep(SLEEP) between polls); after
// ~10 s it stores `code` into the error word and gives up, so the caller proceeds
template <int SCOPE, int SLEEP>
__device__ __forceinline__ void spin_until(const uint32_t* flag, uint32_t e, int* err, int code) {
  const uint64_t t0 = wall_clock();
  while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, SCOPE) < e) {
    __builtin_amdgcn_s_sleep(SLEEP);
    if (wall_clock() - t0 > 1000000000ull) {  // ~10 s at 100 MHz
      atomicExch(err, code);
      break;
    }
  }
}

// The rank-order sums every replica computes alike.  fp32: s = x[0]; s += x[p].  bf16: a = 0; a += float(x[p])
// (the caller rounds a once, or not at all).  Each over the peers' halves at byte offset `off`, piece i, or over
// pieces already in registers (v[p], p < world <= N).
__device__ __forceinline__ void add8(float (&a)[8], const bf16x8& v) {
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] += (float)v[e];
}

__device__ __forceinline__ f32x4 rank_sum_f32(const PeerTable& t, long off, long i, int world) {
  f32x4 s = ((const f32x4*)(t.base[0] + off))[i];
  for (int p = 1; p < world; ++p) s += ((const f32x4*)(t.base[p] + off))[i];
  return s;
}

template <int N>
__device__ __forceinline__ f32x4 rank_sum_f32(const f32x4 (&v)[N], int world) {
  f32x4 s = v[0];
#pragma unroll
  for (int p = 1; p < N; ++p)
    if (p < world) s += v[p];
  return s;
}

__device__ __forceinline__ void rank_sum_bf16(float (&a)[8], const PeerTable& t, long off, long i, int world) {
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = 0.f;
  for (int p = 0; p < world; ++p) add8(a, ((const bf16x8*)(t.base[p] + off))[i]);
}

template <int N>
__device__ __forceinline__ void rank_sum_bf16(float (&a)[8], const bf16x8 (&v)[N], int world) {
  float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // (a local: 2 VGPRs fewer in dp_reduce_shard_kernel<true>)
#pragma unroll
  for (int p = 0; p < N; ++p)
    if (p < world) add8(s, v[p]);
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = s[e];
}

// the exact fp32 images (bits << 16) of the 8 bf16 values of a 16-byte piece: lo = values 0 .. 3, hi = 4 .. 7
__device__ __forceinline__ void widen_bf16x8(const u32x4& v, u32x4& lo, u32x4& hi) {
  lo = u32x4{v[0] << 16, v[0] & 0xffff0000u, v[1] << 16, v[1] & 0xffff0000u};
  hi = u32x4{v[2] << 16, v[2] & 0xffff0000u, v[3] << 16, v[3] & 0xffff0000u};
}

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
    spin_until<__HIP_MEMORY_SCOPE_SYSTEM, 2>((const uint32_t*)t.base[rank] + p, e, err, ERR_BARRIER + p);
  }
  __syncthreads();
  if (p == 0) epoch[0] = e;
}

// copy n16 16-byte pieces of x (any element type) into own half h at piece offset `at` (h read from the epoch
// counter parity: 2 barriers per call): a whole message at 0, or the all-gather's slot
__global__ void p2p_stage16_kernel(const u32x4* __restrict__ x, PeerTable t, int rank, long at, long n16,
                                   long half_bytes, const uint32_t* __restrict__ epoch) {
  const int h = (epoch[0] >> 1) & 1;
  DTC_ASSERT(16 * (at + n16) <= half_bytes && rank >= 0);
  u32x4* dst = (u32x4*)(t.base[rank] + FLAG_BYTES + h * half_bytes) + at;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (long)gridDim.x * blockDim.x) dst[i] = x[i];
}

__global__ void p2p_reduce_scatter_kernel(PeerTable t, int rank, int world, long n4, long half_bytes,
                                          const uint32_t* __restrict__ epoch) {
  const int h = ((epoch[0] - 1) >> 1) & 1;  // one barrier has passed since the stage
  const long chunk = (n4 + world - 1) / world;
  const long lo = rank * chunk, hi = min(n4, lo + chunk);
  const long off = FLAG_BYTES + h * half_bytes;
  DTC_ASSERT(16 * n4 <= half_bytes && rank < world);
  for (long i = lo + (long)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (long)gridDim.x * blockDim.x)
    ((f32x4*)(t.base[rank] + off))[i] = rank_sum_f32(t, off, i, world);
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
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x)
    out[i] = rank_sum_f32(t, off, i, world);
}

// ---------------------------------------------------------------- bf16 payload (tp_comm_dtype: bf16)
// Row-parallel partials travel as bf16 (half the xGMI bytes of the fp32 residual), are summed in fp32
// in rank order, and the LAST kernel adds the fp32 residual and the bias:
//   out[i] = resid[i] + bias[i % ncols] + sum_p partial_p[i]
// so the residual stream itself is never rounded (only the layer's delta is, once, to bf16).  The
// two-shot reduce-scatter stores its reduced slice in bf16 (the all-gather reads half the bytes).

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
    float a[8];
    rank_sum_bf16(a, t, off, i, world);
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
    float a[8];
    rank_sum_bf16(a, t, off, i, world);
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
    const bf16x8 v[1] = {((const bf16x8*)(t.base[(int)(i / chunk)] + off))[i]};  // the slice owner's reduced piece
    float a[8];
    rank_sum_bf16(a, v, 1);
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
    if constexpr (BF16) {
      rank_sum_bf16(a, t, off, lo8 + i, world);
    } else {  // fp32 partials: summed from 0 like the bf16 ones (not from x[0])
      for (int p = 0; p < world; ++p) {
        const f32x4* src = (const f32x4*)(t.base[p] + off) + 2 * (lo8 + i);
        const f32x4 v0 = src[0], v1 = src[1];
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[e] += v0[e]; a[e + 4] += v1[e]; }
      }
    }
    finish8(a, i, out, resid, bias, ncols);  // i indexes this rank's rows: column = (8 i) % ncols
  }
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
  if (threadIdx.x == 0) spin_until<__HIP_MEMORY_SCOPE_SYSTEM, 2>(flags + flag_idx, epoch[0], err, ERR_PP + flag_idx);
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
    if constexpr (F32) widen_bf16x8(v, out_f32[2 * i], out_f32[2 * i + 1]);
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

// The load phase of dp_reduce_kernel and dp_reduce_shard_kernel: all W peers' loads of DP_RU pieces (i0 + u stride,
// below hi) before the first add
template <class V>
__device__ __forceinline__ void dp_load_peers(V (&v)[DP_RU][P2P_MAX], const PeerTable& t, long off, long i0,
                                              long stride, long hi, int world) {
#pragma unroll
  for (int u = 0; u < DP_RU; ++u) {
    const long i = i0 + u * stride;
    if (i < hi) {
#pragma unroll
      for (int p = 0; p < P2P_MAX; ++p)
        if (p < world) v[u][p] = ((const V*)(t.base[p] + off))[i];
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
    dp_load_peers(v, t, off, i0, stride, hi, world);
#pragma unroll
    for (int u = 0; u < DP_RU; ++u) {
      const long i = i0 + u * stride;
      if (i < hi) {
        if constexpr (BF16) {
          float a[8];
          rank_sum_bf16(a, v[u], world);
          bf16x8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = f2bf(a[e]);
          ((bf16x8*)(t.base[rank] + off))[i] = o;
        } else {
          ((f32x4*)(t.base[rank] + off))[i] = rank_sum_f32(v[u], world);
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
          u32x4 hi;
          widen_bf16x8(v[u], out4[2 * i], hi);
          // the last piece of n % 8 == 4 holds 4 elements: never write past out + n
          if (8 * i + 4 < n) out4[2 * i + 1] = hi;
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
//                    of dp_reduce_kernel (dp_load_peers, rank_sum_*), but the result goes as fp32 straight into
//                    grads[own slice] (bf16 widened exactly), so those elements hold bit for bit what
//                    dtc_dp_allreduce would have left there, and
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
    dp_load_peers(v, t, off, i0, stride, hi, world);
#pragma unroll
    for (int u = 0; u < DP_RU; ++u) {
      const long i = i0 + u * stride;
      if (i < hi) {
        if constexpr (BF16) {
          float a[8];
          rank_sum_bf16(a, v[u], world);
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
          const f32x4 s = rank_sum_f32(v[u], world);
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
  if (threadIdx.x == 0) spin_until<__HIP_MEMORY_SCOPE_AGENT, 1>(flags + k, epoch[0], err, ERR_FLAG + k);
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

// ---------------------------------------------------------------- host-side helpers of the entry points
inline PeerTable make_peer_table(void* const* bases, int world) {
  PeerTable t;
  for (int p = 0; p < P2P_MAX; ++p) t.base[p] = (unsigned char*)(p < world ? bases[p] : nullptr);
  return t;
}

// blocks of 256 threads for n items, one each, at least 1 and at most cap
inline int grid_for(long n, long cap = 1024) { return (int)std::min(cap, std::max(1L, (n + 255) / 256)); }

// launch, and return a launch error from the entry point
#define P2P_LAUNCH(K, blocks, threads, st, ...)                             \
  do {                                                                      \
    hipLaunchKernelGGL(K, dim3(blocks), dim3(threads), 0, st, __VA_ARGS__); \
    DTC_CHECK_LAUNCH();                                                     \
  } while (0)
// ... K<true> or K<false> (mostly: a bf16 payload or not), 256 threads
#define P2P_LAUNCH_IF(flag, K, blocks, st, ...)                    \
  do {                                                             \
    if (flag) P2P_LAUNCH(K<true>, blocks, 256, st, __VA_ARGS__);   \
    else P2P_LAUNCH(K<false>, blocks, 256, st, __VA_ARGS__);       \
  } while (0)

// The launches of an all-reduce of `pieces` 16-byte pieces, fp32 and bf16 alike: the stage copy of x (if any), then
// one-shot (barrier + 2, `oneshot`) or two-shot (barrier, `reduce_scatter` over pieces / W, barrier, `all_gather`).
// Both finishing kernels take (t, world, pieces, half_bytes, tail...).
template <class RS, class Fin, class... Tail>
int allreduce_launches(RS* reduce_scatter, Fin* oneshot, Fin* all_gather, const void* x, long pieces, bool one,
                       const PeerTable& t, int rank, int world, long half_bytes, uint32_t* epoch, int* err,
                       hipStream_t st, Tail... tail) {
  const int blocks = grid_for(pieces);
  if (x) P2P_LAUNCH(p2p_stage16_kernel, blocks, 256, st, (const u32x4*)x, t, rank, 0L, pieces, half_bytes, epoch);
  P2P_LAUNCH(p2p_barrier_kernel, 1, 64, st, t, rank, world, epoch, err, one ? 2 : 1);
  if (!one) {
    P2P_LAUNCH(reduce_scatter, grid_for(pieces / world), 256, st, t, rank, world, pieces, half_bytes, epoch);
    P2P_LAUNCH(p2p_barrier_kernel, 1, 64, st, t, rank, world, epoch, err, 1);
  }
  Fin* finish = one ? oneshot : all_gather;
  P2P_LAUNCH(finish, blocks, 256, st, t, world, pieces, half_bytes, tail...);
  return 0;
}

}  // namespace

extern "C" {

int dtc_epoch_inc(uint32_t* epoch, hipStream_t st) {
  P2P_LAUNCH(epoch_inc_kernel, 1, 64, st, epoch);
  return 0;
}

int dtc_flag_set(uint32_t* flags, int k, const uint32_t* epoch, hipStream_t st) {
  P2P_LAUNCH(flag_set_kernel, 1, 64, st, flags, k, epoch);
  return 0;
}

int dtc_flag_wait(const uint32_t* flags, int k, const uint32_t* epoch, int* err, hipStream_t st) {
  P2P_LAUNCH(flag_wait_kernel, 1, 64, st, flags, k, epoch, err);
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
  const bool one = mode == 2 || (mode == 0 && oneshot_auto(n * 4, world));
  return allreduce_launches(p2p_reduce_scatter_kernel, p2p_oneshot_kernel, p2p_all_gather_kernel, x, n / 4, one,
                            make_peer_table(bases, world), rank, world, half_bytes, epoch, err, st, (f32x4*)out,
                            (const uint32_t*)epoch);
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
  const bool one = mode == 2 || (mode == 0 && oneshot_auto(n * 2, world));
  return allreduce_launches(p2p_reduce_scatter_bf16_kernel, p2p_oneshot_bf16_kernel, p2p_all_gather_bf16_kernel, x,
                            n / 8, one, make_peer_table(bases, world), rank, world, half_bytes, epoch, err, st, out,
                            resid, bias, ncols, (const uint32_t*)epoch);
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
  const PeerTable t = make_peer_table(bases, world);
  const long n16 = n_loc * world * esz / 16, n8 = n_loc / 8;
  if (x) P2P_LAUNCH(p2p_stage16_kernel, grid_for(n16), 256, st, (const u32x4*)x, t, rank, 0L, n16, half_bytes, epoch);
  P2P_LAUNCH(p2p_barrier_kernel, 1, 64, st, t, rank, world, epoch, err, 2);
  P2P_LAUNCH_IF(bf16, p2p_rs_kernel, grid_for(n8), st, t, rank, world, n8, half_bytes, out, resid, bias, ncols,
                  epoch);
  return 0;
}

// all-gather of this rank's loc_bytes (x, a multiple of 16) into out [W * loc_bytes], rank-major.
// x == nullptr: the producer already wrote the slot (staged_out at offset rank * loc_bytes).
int dtc_p2p_all_gather(const void* x, void* out, long loc_bytes, void* const* bases, int rank, int world,
                       long half_bytes, uint32_t* epoch, int* err, hipStream_t st) {
  if (world < 1 || world > P2P_MAX || loc_bytes % 16 || loc_bytes * world > half_bytes) return 4001;
  const PeerTable t = make_peer_table(bases, world);
  const long n16 = loc_bytes / 16;
  if (x)
    P2P_LAUNCH(p2p_stage16_kernel, grid_for(n16), 256, st, (const u32x4*)x, t, rank, rank * n16, n16, half_bytes,
               epoch);
  P2P_LAUNCH(p2p_barrier_kernel, 1, 64, st, t, rank, world, epoch, err, 2);
  P2P_LAUNCH(p2p_ag_kernel, grid_for(n16 * world), 256, st, t, world, n16, half_bytes, (u32x4*)out, epoch);
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
  if (x)
    P2P_LAUNCH(pp_stage_kernel, grid_for(n / 16), 256, st, (const u32x4*)x,
               (u32x4*)((unsigned char*)own_base + FLAG_BYTES + slot_off), n / 16, slot_off, buf_bytes);
  P2P_LAUNCH(pp_signal_kernel, 1, 64, st, (uint32_t*)peer_base, flag_idx, epoch);
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
  P2P_LAUNCH(pp_wait_kernel, 1, 64, st, (const uint32_t*)own_base, flag_idx, epoch, err);
  const u32x4* slot = (const u32x4*)((const unsigned char*)peer_base + FLAG_BYTES + slot_off);
  P2P_LAUNCH_IF(out_f32 != nullptr, pp_pull_kernel, grid_for(n / 16), st, slot, (u32x4*)out, (u32x4*)out_f32, n / 16,
                  slot_off, buf_bytes);
  return 0;
}

// ---- DP gradient buckets (kernels above): grads[0:n] (fp32, 16-byte aligned, n a positive multiple of 4) =
// sum over ranks, in place.  bf16: the payload travels as bf16 (fp32 sums in rank order, one rounding of the
// reduced slice); ceil(n / 8) 16-byte pieces must fit the half, else n / 4.  Every grid is at most max_blocks
// blocks (1 .. 1024).  Epoch + 2 like every other call on the object.
// What the three bucket calls require of their common arguments (buf: the fp32 bucket, grads or params)
inline bool dp_args_ok(const float* buf, long n, void* const* bases, int rank, int world, long half_bytes,
                       const uint32_t* epoch, const int* err, int max_blocks) {
  return buf && bases && epoch && err && world >= 1 && world <= P2P_MAX && rank >= 0 && rank < world && n > 0 &&
         n % 4 == 0 && !((uintptr_t)buf & 15) && max_blocks >= 1 && max_blocks <= 1024 && half_bytes > 0 &&
         half_bytes % 16 == 0;
}
inline long dp_pieces(long n, int bf16) { return bf16 ? (n + 7) / 8 : n / 4; }  // 16-byte pieces of the payload

int dtc_dp_allreduce(float* grads, long n, int bf16, void* const* bases, int rank, int world, long half_bytes,
                     uint32_t* epoch, int* err, int max_blocks, hipStream_t st) {
  if (!dp_args_ok(grads, n, bases, rank, world, half_bytes, epoch, err, max_blocks)) return 4001;
  const long pieces = dp_pieces(n, bf16);
  if (pieces > half_bytes / 16) return 4001;
  const PeerTable t = make_peer_table(bases, world);
  const long chunk = (pieces + world - 1) / world;
  const int blocks = grid_for(pieces, max_blocks);
  P2P_LAUNCH_IF(bf16, dp_pack_kernel, blocks, st, grads, t, rank, n, pieces, half_bytes, epoch);
  P2P_LAUNCH(p2p_barrier_kernel, 1, 64, st, t, rank, world, epoch, err, 1);
  P2P_LAUNCH_IF(bf16, dp_reduce_kernel, grid_for(chunk, max_blocks), st, t, rank, world, pieces, half_bytes, epoch);
  P2P_LAUNCH(p2p_barrier_kernel, 1, 64, st, t, rank, world, epoch, err, 1);
  P2P_LAUNCH_IF(bf16, dp_gather_kernel, blocks, st, t, world, n, pieces, half_bytes, grads, epoch);
  return 0;
}

// ---- ZeRO-1 over the DP buckets (kernels above).  Both calls: epoch + 2, one barrier.
// Blocks (= Σg² partial slots) of the reduce-scatter of an n-element bucket; the same on every rank.
int dtc_dp_rs_slots(long n, int bf16, int world, int max_blocks) {
  if (n <= 0 || n % 4 || world < 1 || world > P2P_MAX || max_blocks < 1 || max_blocks > 1024) return -1;
  return grid_for((dp_pieces(n, bf16) + world - 1) / world, max_blocks);
}

// grads[own slice] (fp32, in place) = sum over ranks of grads[own slice], where the own slice of the n-element
// bucket is pieces [min(pieces, rank chunk), min(pieces, (rank + 1) chunk)) of 4 fp32 / 8 bf16 elements, chunk =
// ceil(pieces / W): the values dtc_dp_allreduce leaves there.  Nothing else of grads is written.  part[0 : nslots]
// (nslots == dtc_dp_rs_slots(...)) = per-block partial sums of squares of the slice (zeros for an empty one).
int dtc_dp_reduce_scatter(float* grads, long n, int bf16, float* part, int nslots, void* const* bases, int rank,
                          int world, long half_bytes, uint32_t* epoch, int* err, int max_blocks, hipStream_t st) {
  if (!dp_args_ok(grads, n, bases, rank, world, half_bytes, epoch, err, max_blocks) || !part || ((uintptr_t)part & 3))
    return 4001;
  const long pieces = dp_pieces(n, bf16);
  if (pieces > half_bytes / 16 || nslots != dtc_dp_rs_slots(n, bf16, world, max_blocks)) return 4001;
  const PeerTable t = make_peer_table(bases, world);
  P2P_LAUNCH_IF(bf16, dp_pack_kernel, grid_for(pieces, max_blocks), st, grads, t, rank, n, pieces, half_bytes, epoch);
  P2P_LAUNCH(p2p_barrier_kernel, 1, 64, st, t, rank, world, epoch, err, 2);
  P2P_LAUNCH_IF(bf16, dp_reduce_shard_kernel, nslots, st, t, rank, world, n, pieces, half_bytes, grads, part, epoch);
  return 0;
}

// params[0:n] (fp32, one bucket) = every rank's owned slice of it (the ownership of dtc_dp_reduce_scatter with the
// same n, bf16 and world; bf16 only selects that plan, the parameters travel as fp32), own slice untouched;
// mirror[0:n_mirror] (bf16, optional, n_mirror <= n) = the rounded parameters, in the same pass.  Grids of at most
// max_blocks (1 .. 1024; the step's tail, nothing overlaps it: the caller passes 1024).
int dtc_dp_param_gather(float* params, bf16* mirror, long n, long n_mirror, int bf16_plan, void* const* bases,
                        int rank, int world, long half_bytes, uint32_t* epoch, int* err, int max_blocks,
                        hipStream_t st) {
  if (!dp_args_ok(params, n, bases, rank, world, half_bytes, epoch, err, max_blocks) || ((uintptr_t)mirror & 7) ||
      n_mirror < 0 || n_mirror > n || n_mirror % 4 || (n_mirror > 0 && !mirror))
    return 4001;
  const int qpp = bf16_plan ? 2 : 1;
  const long nq = n / 4, pieces = (nq + qpp - 1) / qpp;
  const long chunk = (pieces + world - 1) / world;
  if (std::min(nq, chunk * qpp) > half_bytes / 16) return 4001;  // the largest slice (rank 0's) must fit the half
  const long q_lo = std::min(nq, rank * chunk * qpp), q_hi = std::min(nq, q_lo + chunk * qpp);
  const PeerTable t = make_peer_table(bases, world);
  P2P_LAUNCH(dp_pack_params_kernel, grid_for(q_hi - q_lo, max_blocks), 256, st, params, t, rank, q_lo, q_hi, half_bytes,
             epoch);
  P2P_LAUNCH(p2p_barrier_kernel, 1, 64, st, t, rank, world, epoch, err, 2);
  P2P_LAUNCH(dp_gather_params_kernel, grid_for(nq, max_blocks), 256, st, t, rank, world, n, pieces, qpp, half_bytes,
             params, mirror, n_mirror, epoch);
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
  P2P_LAUNCH(p2p_barrier_kernel, 1, 64, st, make_peer_table(bases, world), rank, world, epoch, err, 2);
  return 0;
}

}  // extern "C"
