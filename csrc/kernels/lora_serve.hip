// Multi-adapter LoRA for serving: every row of a decode batch adds the delta of ITS OWN adapter,
//     y[b, n] += s[id_b] * sum_j (sum_k x[b, k] A[id_b, j, k]) * B[id_b, n, j],
// in two launches per projection, no atomics and no arrival counters (mxllm/ops/lora_serve.py).
//
// Tables of one projection (allocated once, every adapter slot zero-padded to r_max):
//   A_tab bf16 [n_adapters, R, K], R = n_splits * r_max: the splits' A matrices stacked
//   B_tab bf16 [n_adapters, N, r_max]: row n holds the r_max columns of n's own split (B is
//         block-diagonal, so the other columns are zero and are not stored)
//   s_tab f32  [n_adapters]: alpha / r
//   ids   int32 [M]: the adapter of each row, -1 = none (the row is neither read nor written)
//
//  * lora_shrink_kernel, grid (M, KS, ceil(R / 16)), KS = ceil(K / 512): a workgroup takes 16 table
//    rows, 4 per wave; lane l holds x[b, ks * 512 + 8 l ..+8) (one 16-B load, zero past K),
//    multiplies it with the same 8 columns of A row j (one 16-B load) by 8 fmas in ascending k,
//    and the 64 lane sums are added by the xor butterfly 32, 16, ..., 1.  partials[ks, b, j] f32.
//    A wave issues its five loads together; a decode row is bound by latency, not bytes.
//  * lora_expand_kernel, grid (M, ceil(N / 2048)): t[j] = partials[0, b, j] + partials[1, b, j] +
//    ... in ascending ks (fp32, staged through LDS 1024 partials at a time); each thread then owns
//    8 consecutive n (one 16-B access to y; 8 | every split, so they share a split):
//        acc = fma(t[j], B[n, j], acc) for j = 0 .. r_max - 1 of n's split, acc = 0 first
//        y[b, n] = bf16(fma(s, acc, f32(y[b, n])))
//
// The order of every sum is fixed by K and the constants above: it depends neither on M nor on
// another row's id, so a row gives the same bits alone and inside any batch.  Nothing is read on
// the host and nothing allocated, so both launches can be captured in a graph.  Rows that share an
// adapter re-read its tables from L2.
#include "bindings.h"
#include "common.h"

namespace mx {

namespace {

constexpr int kLsChunk = 512;  // K columns per shrink workgroup: 64 lanes x 8 bf16
constexpr int kLsMaxR = 192;   // 3 splits x r_max 64
constexpr int kLsRows = 16;    // table rows per shrink workgroup: 4 per wave
constexpr int kLsTile = 1024;  // partials the expand kernel stages in LDS at a time

__global__ void __launch_bounds__(256) lora_shrink_kernel(const uint16_t* __restrict__ x, int64_t ldx,
                                                          const int32_t* __restrict__ ids,
                                                          const uint16_t* __restrict__ a_tab,
                                                          float* __restrict__ part, int M, int K, int R,
                                                          int n_adapters) {
  const int b = blockIdx.x, ks = blockIdx.y;
  const int id = ids[b];
  if (id < 0 || id >= n_adapters) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = ks * kLsChunk + lane * 8;
  const bool live = k < K;  // K % 8 == 0: a vector is whole or absent
  const int j0 = blockIdx.z * kLsRows + wave * (kLsRows / 4);
  const uint16_t* a = a_tab + ((int64_t)id * R + j0) * K + k;
  // the x chunk and this wave's table rows are all requested before the first is used: a row's
  // latency is one trip to memory, not one per table row
  const u16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  u16x8 xv = zero, av[kLsRows / 4];
  if (live) xv = *reinterpret_cast<const u16x8*>(x + (int64_t)b * ldx + k);
#pragma unroll
  for (int i = 0; i < kLsRows / 4; ++i) {
    av[i] = zero;
    if (live && j0 + i < R) av[i] = *reinterpret_cast<const u16x8*>(a + (int64_t)i * K);
  }
  float* out = part + ((int64_t)ks * M + b) * R;
#pragma unroll
  for (int i = 0; i < kLsRows / 4; ++i) {
    float acc = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = __builtin_fmaf(bf2f(xv[e]), bf2f(av[i][e]), acc);
    acc = wave_sum(acc);
    if (lane == 0 && j0 + i < R) out[j0 + i] = acc;
  }
}

template <int RMAX>
__global__ void __launch_bounds__(256) lora_expand_kernel(uint16_t* __restrict__ y, int64_t ldy,
                                                          const float* __restrict__ part,
                                                          const int32_t* __restrict__ ids,
                                                          const uint16_t* __restrict__ b_tab,
                                                          const float* __restrict__ s_tab, int M, int N, int R, int KS,
                                                          int e0, int e1, int n_adapters) {
  __shared__ float t[kLsMaxR];
  __shared__ float pt[kLsTile];
  const int b = blockIdx.x;
  const int id = ids[b];
  if (id < 0 || id >= n_adapters) return;  // the whole workgroup leaves: no barrier is skipped by a part of it
  // t: the partials come to LDS a tile of whole K splits at a time, every thread loading (so the
  // loads of a tile are in flight together); thread j then adds its column in ascending ks
  const int per = kLsTile / R;  // K splits per tile: 5 (R 192) to 128 (R 8)
  float tj = 0.f;
  for (int ks0 = 0; ks0 < KS; ks0 += per) {
    const int nk = min(per, KS - ks0);
    for (int e = threadIdx.x; e < nk * R; e += 256) {
      const int ks = ks0 + e / R;
      pt[e] = part[((int64_t)ks * M + b) * R + (e - (ks - ks0) * R)];
    }
    __syncthreads();
    if (threadIdx.x < R)
      for (int q = 0; q < nk; ++q) tj += pt[q * R + threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x < R) t[threadIdx.x] = tj;
  __syncthreads();
  const int n0 = (blockIdx.y * 256 + threadIdx.x) * 8;
  if (n0 >= N) return;  // N % 8 == 0: the 8 columns are whole or absent
  const float* ts = t + ((n0 >= e0) + (n0 >= e1)) * RMAX;
  const float s = s_tab[id];
  const uint16_t* bp = b_tab + ((int64_t)id * N + n0) * RMAX;
  uint16_t* yp = y + (int64_t)b * ldy + n0;
  const u16x8 yv = *reinterpret_cast<const u16x8*>(yp);
  u16x8 ov;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < RMAX / 8; ++c) {
      const u16x8 bv = *reinterpret_cast<const u16x8*>(bp + i * RMAX + c * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc = __builtin_fmaf(ts[c * 8 + e], bf2f(bv[e]), acc);
    }
    ov[i] = f2bf(__builtin_fmaf(s, acc, bf2f(yv[i])));
  }
  *reinterpret_cast<u16x8*>(yp) = ov;
}

bool ls_rank_ok(int r) { return r == 8 || r == 16 || r == 32 || r == 64; }

}  // namespace

}  // namespace mx

extern "C" {

int mx_lora_serve_ksplits(int K) { return (K + mx::kLsChunk - 1) / mx::kLsChunk; }

int mx_lora_gather_shrink(const uint16_t* x, int64_t ldx, const int32_t* ids, const uint16_t* a_tab, float* part,
                          int M, int K, int R, int n_adapters, hipStream_t stream) {
  if (M < 1 || K < 8 || K % 8 || R < 8 || R % 8 || R > mx::kLsMaxR || ldx < K || ldx % 8 || n_adapters < 1) return -1;
  const int KS = mx_lora_serve_ksplits(K);
  if (KS > 65535) return -1;
  hipLaunchKernelGGL(mx::lora_shrink_kernel, dim3(M, KS, (R + mx::kLsRows - 1) / mx::kLsRows), dim3(256), 0, stream, x,
                     ldx, ids, a_tab, part, M, K, R, n_adapters);
  return (int)hipGetLastError();
}

int mx_lora_gather_expand_add(uint16_t* y, int64_t ldy, const float* part, const int32_t* ids, const uint16_t* b_tab,
                              const float* s_tab, int M, int N, int KS, int r_max, const int* splits, int n_splits,
                              int n_adapters, hipStream_t stream) {
  if (M < 1 || N < 8 || N % 8 || KS < 1 || !mx::ls_rank_ok(r_max) || n_splits < 1 || n_splits > 3 || ldy < N ||
      ldy % 8 || n_adapters < 1)
    return -1;
  int64_t sum = 0;
  for (int i = 0; i < n_splits; ++i) {
    if (splits[i] < 8 || splits[i] % 8) return -1;
    sum += splits[i];
  }
  if (sum != N) return -1;
  const int e0 = n_splits > 1 ? splits[0] : 0x7fffffff;
  const int e1 = n_splits > 2 ? splits[0] + splits[1] : 0x7fffffff;
  const int R = n_splits * r_max;
  const dim3 grid(M, (N + 2047) / 2048);
  if (grid.y > 65535) return -1;
#define MX_LS_EXPAND(RM)                                                                                            \
  hipLaunchKernelGGL(mx::lora_expand_kernel<RM>, grid, dim3(256), 0, stream, y, ldy, part, ids, b_tab, s_tab, M, N, \
                     R, KS, e0, e1, n_adapters)
  switch (r_max) {
    case 8: MX_LS_EXPAND(8); break;
    case 16: MX_LS_EXPAND(16); break;
    case 32: MX_LS_EXPAND(32); break;
    default: MX_LS_EXPAND(64); break;
  }
#undef MX_LS_EXPAND
  return (int)hipGetLastError();
}
}
