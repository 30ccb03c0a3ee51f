// Logits processing beside the sampler (serving): sampling penalties + logit_bias, the
// per-request token counts they need, and log-probabilities of the chosen / top-n tokens.
// All three run outside the captured decode graph, on the [B, V] logits that never leave
// the GPU (OpenAI presence / frequency penalty, logit_bias, logprobs / top_logprobs; the
// HF / vLLM repetition penalty).
//
//  * logits_adjust_kernel: elementwise, f32 out.  Per element, in this order, every
//    operation rounded on its own (nothing contracts, so the result equals the same
//    expression written in fp32 PyTorch bit for bit):
//        x = float(logit)
//        seen (prompt flag or count > 0) and repetition != 1:  x = x > 0 ? x / rep : x * rep
//        count c > 0:                                          x = x - (freq * float(c) + pres)
//        bias != 0:                                            x = x + bias
//    An element none of these touches is the converted input, sign of zero included.
//  * token_state_kernel: count[slot, id] += 1 for the tokens just drawn.
//  * logprob_slice_kernel + logprob_merge_kernel: fp32 log-softmax of the chosen and the n
//    most likely tokens per row (ties to the lower index, the sampler's greedy rule); see
//    the comment above them.
//
// token state: int32 [n_slots, V]; bits 0..30 = occurrences in the request's output,
// bit 31 = "occurs in the prompt".
#include "bindings.h"
#include "common.h"

namespace mx {

namespace {

constexpr int kTopMax = 20;

// compiler barrier on a value: the product / sum that went in cannot fuse with its consumer
__device__ __forceinline__ float lp_pin(float x) {
  asm volatile("" : "+v"(x));
  return x;
}

__device__ __forceinline__ uint32_t lp_okey(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float lp_key2f(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ float adjust_one(float x, int32_t st, float pres, float freq, float rep, float bias) {
#pragma clang fp contract(off)
  const int32_t c = st & 0x7fffffff;
  if (st != 0 && rep != 1.f) x = x > 0.f ? lp_pin(__fdiv_rn(x, rep)) : lp_pin(__fmul_rn(x, rep));
  if (c > 0) {
    const float fc = lp_pin(__fmul_rn(freq, (float)c));
    const float pen = lp_pin(__fadd_rn(fc, pres));
    x = lp_pin(__fsub_rn(x, pen));
  }
  if (bias != 0.f) x = lp_pin(__fadd_rn(x, bias));
  return x;
}

template <typename T>
__device__ __forceinline__ float ld1(const T* p, int64_t i) {
  if constexpr (sizeof(T) == 2) return bf2f(reinterpret_cast<const uint16_t*>(p)[i]);
  else return reinterpret_cast<const float*>(p)[i];
}

// grid (B, ceil(V / (256 * 4))); 4 elements per thread, 16-B accesses when the rows allow
template <typename T>
__global__ void __launch_bounds__(256) logits_adjust_kernel(
    const T* __restrict__ logits, float* __restrict__ out, int V, const int32_t* __restrict__ state,
    const int32_t* __restrict__ slots, int n_slots, const float* __restrict__ pres, const float* __restrict__ freq,
    const float* __restrict__ rep, const float* __restrict__ bias) {
  const int row = blockIdx.x;
  const int64_t off = (int64_t)row * V;
  const int j0 = (blockIdx.y * 256 + threadIdx.x) * 4;
  if (j0 >= V) return;
  const int slot = slots[row];
  const bool live = slot >= 0 && slot < n_slots;
  const int32_t* st = (live && state) ? state + (int64_t)slot * V : nullptr;
  const float* bs = (live && bias) ? bias + (int64_t)slot * V : nullptr;
  const float p = pres[row], f = freq[row], r = rep[row];
  // every row starts at a multiple of V elements: 4-element vectors are aligned when V % 4 == 0
  // and the base pointers are
  const bool vec = (V & 3) == 0 && j0 + 4 <= V && ((((uintptr_t)logits) | ((uintptr_t)out) | ((uintptr_t)state) |
                                                    ((uintptr_t)bias)) & 15) == 0;
  float x[4];
  int32_t s[4] = {0, 0, 0, 0};
  float b[4] = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    if constexpr (sizeof(T) == 2) {
      const u16x4 v = *reinterpret_cast<const u16x4*>(reinterpret_cast<const uint16_t*>(logits) + off + j0);
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = bf2f(v[k]);
    } else {
      const f32x4 v = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(logits) + off + j0);
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = v[k];
    }
    if (st) {
      const int4 v = *reinterpret_cast<const int4*>(st + j0);
      s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
    }
    if (bs) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(bs + j0);
#pragma unroll
      for (int k = 0; k < 4; ++k) b[k] = v[k];
    }
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = adjust_one(x[k], s[k], p, f, r, b[k]);
    *reinterpret_cast<f32x4*>(out + off + j0) = o;
    return;
  }
  for (int k = 0; k < 4 && j0 + k < V; ++k) {
    const float xv = ld1(logits, off + j0 + k);
    out[off + j0 + k] = adjust_one(xv, st ? st[j0 + k] : 0, p, f, r, bs ? bs[j0 + k] : 0.f);
  }
}

__global__ void token_state_kernel(int32_t* __restrict__ state, const int32_t* __restrict__ slots,
                                   const int64_t* __restrict__ ids, int B, int V, int n_slots) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int slot = slots[b];
  const int64_t id = ids[b];
  if (slot < 0 || slot >= n_slots || id < 0 || id >= V) return;
  atomicAdd(&state[(int64_t)slot * V + id], 1);
}

// ---- log-probabilities: slice pass, then merge -------------------------------------------------
// A row is cut into slices of kSlice elements, one wavefront each (grid: slices x rows).  The
// wave holds its slice in registers as order-preserving 32-bit keys (32 per lane), so after
// the one read of the row everything is register arithmetic and wave shuffles: the slice
// maximum, sum exp(x - max) and the slice's n_top largest elements as 64-bit keys
// (okey(x) << 32) | ~index, found by n_top rounds of "wave argmax, winner drops its element".
// The merge kernel (one wave per row) combines the slices' (max, sum) into the row's lse and
// picks the n_top largest of the slices' candidates the same way, from LDS.  The global top n
// is a subset of the union of the slices' top n, every key is distinct, and all sums run in a
// fixed order: exact and deterministic.
constexpr int kSlice = 2048;         // elements per wave: 32 per lane
constexpr int kPerLane = kSlice / 64;
constexpr int kMaxSlices = 400;      // merge kernel LDS: 400 * 20 keys * 8 B = 64,000 B

__device__ __forceinline__ uint32_t lp_okey0(float v) {
  if (v == 0.f) v = 0.f;  // -0.0 ties with +0.0
  return lp_okey(v);
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)k, o, 64), hi = __shfl_xor((uint32_t)(k >> 32), o, 64);
    const uint64_t other = ((uint64_t)hi << 32) | lo;
    k = other > k ? other : k;
  }
  return k;
}

// ws_keys [B, S, 20] (first n_top[row] entries of each slice written, 0 = none),
// ws_stat [B, S, 2] = (slice max, sum exp(x - slice max))
template <typename T>
__global__ void __launch_bounds__(64) logprob_slice_kernel(const T* __restrict__ logits,
                                                           const int32_t* __restrict__ n_top,
                                                           uint64_t* __restrict__ ws_keys,
                                                           float* __restrict__ ws_stat, int V, int S) {
  const int row = blockIdx.y, sl = blockIdx.x, lane = threadIdx.x;
  int n = n_top[row];
  if (n < 0) return;
  n = min(n, kTopMax);
  const int base = sl * kSlice;
  const int len = min(kSlice, V - base);  // >= 1
  const T* x = logits + (int64_t)row * V + base;
  // element i of this lane sits at slice offset off(i), increasing in i; 0 = no element
  uint32_t k[kPerLane];
  constexpr int kVec = 16 / sizeof(T);  // elements per 16-B load
  const bool vec = (((uintptr_t)x) & 15) == 0;
  if (vec) {
#pragma unroll
    for (int q = 0; q < kPerLane / kVec; ++q) {
      const int o = q * 64 * kVec + lane * kVec;
      if (o + kVec <= len) {
        if constexpr (sizeof(T) == 2) {
          const u16x8 v = *reinterpret_cast<const u16x8*>(reinterpret_cast<const uint16_t*>(x) + o);
#pragma unroll
          for (int j = 0; j < kVec; ++j) k[q * kVec + j] = lp_okey0(bf2f(v[j]));
        } else {
          const f32x4 v = *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(x) + o);
#pragma unroll
          for (int j = 0; j < kVec; ++j) k[q * kVec + j] = lp_okey0(v[j]);
        }
      } else {
#pragma unroll
        for (int j = 0; j < kVec; ++j) k[q * kVec + j] = o + j < len ? lp_okey0(ld1(x, o + j)) : 0u;
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < kPerLane; ++i) k[i] = i * 64 + lane < len ? lp_okey0(ld1(x, i * 64 + lane)) : 0u;
  }
  uint64_t* keys = ws_keys + ((int64_t)row * S + sl) * kTopMax;
  for (int t = 0; t < max(n, 1); ++t) {
    uint32_t bk = 0;
    int bi = 0;
#pragma unroll
    for (int i = 0; i < kPerLane; ++i)
      if (k[i] > bk) { bk = k[i]; bi = i; }  // first of equals: the lower index
    const int off = vec ? (bi / kVec) * 64 * kVec + lane * kVec + bi % kVec : bi * 64 + lane;
    const uint64_t mine = bk ? ((uint64_t)bk << 32) | (uint32_t)~(uint32_t)(base + off) : 0ull;
    const uint64_t win = wave_max_u64(mine);
    if (t == 0) {  // the slice maximum: sum exp(x - max) before anything is dropped
      const float mx = lp_key2f((uint32_t)(win >> 32));
      float z = 0.f;
#pragma unroll
      for (int i = 0; i < kPerLane; ++i)
        if (k[i]) z += expf(lp_key2f(k[i]) - mx);
      z = wave_sum(z);
      if (lane == 0) {
        ws_stat[((int64_t)row * S + sl) * 2] = mx;
        ws_stat[((int64_t)row * S + sl) * 2 + 1] = z;
      }
    }
    if (t < n && lane == 0) keys[t] = win;
    if (win != 0 && mine == win) {
#pragma unroll
      for (int i = 0; i < kPerLane; ++i) k[i] = i == bi ? 0u : k[i];
    }
  }
}

template <typename T>
__global__ void __launch_bounds__(64) logprob_merge_kernel(
    const T* __restrict__ logits, const int64_t* __restrict__ ids, const int32_t* __restrict__ n_top,
    const uint64_t* __restrict__ ws_keys, const float* __restrict__ ws_stat, float* __restrict__ chosen_lp,
    int32_t* __restrict__ top_ids, float* __restrict__ top_lp, int V, int S) {
  extern __shared__ uint64_t cand[];  // [S * n]
  const int row = blockIdx.x, lane = threadIdx.x;
  int n = n_top[row];
  if (lane < kTopMax) {
    top_ids[row * kTopMax + lane] = -1;
    top_lp[row * kTopMax + lane] = -INFINITY;
  }
  if (n < 0) {
    if (lane == 0) chosen_lp[row] = -INFINITY;
    return;
  }
  n = min(n, kTopMax);
  const float* st = ws_stat + (int64_t)row * S * 2;
  float mx = -INFINITY;
  for (int s = lane; s < S; s += 64) mx = fmaxf(mx, st[s * 2]);
  mx = wave_max(mx);
  float z = 0.f;
  for (int s = lane; s < S; s += 64) z += st[s * 2 + 1] * expf(st[s * 2] - mx);
  z = wave_sum(z);
  const float lse = mx + logf(z);
  if (lane == 0) {
    const int64_t id = ids[row];
    float xv = (id >= 0 && id < V) ? ld1(logits, (int64_t)row * V + id) : -INFINITY;
    if (xv == 0.f) xv = 0.f;  // as in the keys
    chosen_lp[row] = xv - lse;
  }
  const int total = S * n;
  const uint64_t* keys = ws_keys + (int64_t)row * S * kTopMax;
  for (int e = lane; e < total; e += 64) cand[e] = keys[(e / n) * kTopMax + e % n];
  // every lane reads and clears only its own entries: no barrier needed
  for (int t = 0; t < n; ++t) {
    uint64_t best = 0;
    int be = -1;
    for (int e = lane; e < total; e += 64) {
      const uint64_t c = cand[e];
      if (c > best) { best = c; be = e; }
    }
    const uint64_t win = wave_max_u64(best);
    if (win == 0) break;
    if (best == win) {
      cand[be] = 0;
      const int idx = (int)~(uint32_t)win;
      top_ids[row * kTopMax + t] = idx;
      top_lp[row * kTopMax + t] = lp_key2f((uint32_t)(win >> 32)) - lse;  // the same expression as chosen_lp
    }
  }
}

}  // namespace
}  // namespace mx

using namespace mx;

// logits [B, V] bf16 (is_bf16) or f32 -> out f32 [B, V].  state int32 [n_slots, V] or null
// (no token seen), bias f32 [n_slots, V] or null; slots int32 [B] (< 0: plain conversion);
// presence / frequency / repetition f32 [B].
extern "C" int mx_logits_adjust_rows(const void* logits, int is_bf16, float* out, int B, int V, const int32_t* state,
                                     const int32_t* slots, int n_slots, const float* presence,
                                     const float* frequency, const float* repetition, const float* bias,
                                     hipStream_t stream) {
  if (B <= 0) return 0;
  if (V <= 0) return -1;
  const dim3 grid(B, (V + 1023) / 1024);
  if (is_bf16)
    logits_adjust_kernel<uint16_t><<<grid, 256, 0, stream>>>((const uint16_t*)logits, out, V, state, slots, n_slots,
                                                             presence, frequency, repetition, bias);
  else
    logits_adjust_kernel<float><<<grid, 256, 0, stream>>>((const float*)logits, out, V, state, slots, n_slots,
                                                          presence, frequency, repetition, bias);
  return (int)hipGetLastError();
}

// state[slots[b], ids[b]] += 1 (rows with slots[b] < 0 skipped)
extern "C" int mx_token_state_update(int32_t* state, const int32_t* slots, const int64_t* ids, int B, int V,
                                     int n_slots, hipStream_t stream) {
  if (B <= 0) return 0;
  if (V <= 0) return -1;
  token_state_kernel<<<(B + 63) / 64, 64, 0, stream>>>(state, slots, ids, B, V, n_slots);
  return (int)hipGetLastError();
}

// bytes of workspace mx_logprob_rows needs for [B, V] logits (per call, owned by the caller)
extern "C" int64_t mx_logprob_ws_bytes(int B, int V) {
  const int64_t S = (V + kSlice - 1) / kSlice;
  return (int64_t)B * S * (kTopMax * 8 + 2 * 4);
}

// logits [B, V] bf16 / f32, ids int64 [B], n_top int32 [B] (-1: skip the row, else 0..20) ->
// chosen_lp f32 [B], top_ids int32 [B, 20] (-1 beyond n_top), top_lp f32 [B, 20] (-inf beyond).
// ws: mx_logprob_ws_bytes(B, V) bytes, 8-B aligned.  V <= 2048 * 400.
extern "C" int mx_logprob_rows(const void* logits, int is_bf16, const int64_t* ids, const int32_t* n_top,
                               float* chosen_lp, int32_t* top_ids, float* top_lp, int B, int V, void* ws,
                               hipStream_t stream) {
  if (B <= 0) return 0;
  const int S = (V + kSlice - 1) / kSlice;
  if (V <= 0 || S > kMaxSlices || B > 65535 || !ws) return -1;
  uint64_t* ws_keys = (uint64_t*)ws;
  float* ws_stat = (float*)(ws_keys + (int64_t)B * S * kTopMax);
  const dim3 grid(S, B);
  const size_t lds = (size_t)S * kTopMax * sizeof(uint64_t);
  if (is_bf16) {
    logprob_slice_kernel<uint16_t><<<grid, 64, 0, stream>>>((const uint16_t*)logits, n_top, ws_keys, ws_stat, V, S);
    logprob_merge_kernel<uint16_t><<<B, 64, lds, stream>>>((const uint16_t*)logits, ids, n_top, ws_keys, ws_stat,
                                                           chosen_lp, top_ids, top_lp, V, S);
  } else {
    logprob_slice_kernel<float><<<grid, 64, 0, stream>>>((const float*)logits, n_top, ws_keys, ws_stat, V, S);
    logprob_merge_kernel<float><<<B, 64, lds, stream>>>((const float*)logits, ids, n_top, ws_keys, ws_stat,
                                                        chosen_lp, top_ids, top_lp, V, S);
  }
  return (int)hipGetLastError();
}
