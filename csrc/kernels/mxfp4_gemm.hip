// MXFP4 (OCP Microscaling v1.0: e2m1 elements, one e8m0 scale per 32 k) weight-only GEMM for decode
// on gfx950: Y[M, N] = X[M, K] . dequant(codes, scales)^T with M <= 32 tokens, bf16 activations /
// output, f32 accumulation.  The decode step is bound by streaming every projection weight once;
// 4-bit weights halve that traffic again against fp8_gemm.hip, on which this kernel is modelled.
// Format and reference: mxllm/serve/quant.py.  Which launches are taken: mx::w4_takes (w4_args.h).
//
// Structure (memory-bound; the MFMA is nearly free):
//  * workgroup = NW waves (8, or 4 where K is no multiple of 1024) x 16 * NC output channels; the
//    waves split K in NW contiguous parts and their partial sums meet in LDS; the k loop issues a
//    batch of chunks' loads before using any;
//  * v_mfma_f32_16x16x32_bf16 with the WEIGHTS as the A operand (16 channels x 32 k) and X^T as
//    the B operand (32 k x 16 tokens): one MFMA chain per (channel group, 16-token block);
//  * a chunk is 128 k.  Lane (c = lane & 15, g = lane >> 4) loads the 16 contiguous code bytes of
//    k = 32g .. 32g + 31 of channel c: exactly one scale block, so one scale byte per load (the
//    four bytes of a chunk are one aligned 32-bit word; the lane takes byte g).  Word s of the
//    load is MFMA k-step s: the chunk's four MFMAs take k = 32g + 8s + j (permuted inside the
//    chunk), and the X fragments use the same permutation (four 16-B bf16 loads per token block);
//  * dequantisation: v_cvt_scalef32_pk_bf16_fp4 (two codes of a selected byte x an f32 scale ->
//    packed bf16), the scale built as byte << 23 = 2^(byte - 127).  Every product grid x 2^e has
//    at most two mantissa bits, so the conversion has nothing to round; the every-code test
//    (tests/test_mxfp4_gpu.py, 16 codes x scale bytes 1..254 x both nibbles) holds it to the
//    reference bit for bit through w4_dequant_kernel, which decodes with the same function.
#include <cstdlib>
#include <type_traits>

#include "bindings.h"
#include "common.h"

namespace mx {

typedef __bf16 bf16x8_w4 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_w4 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_w4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma16_w4(const u16x8& a, const u16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_w4, a), __builtin_bit_cast(bf16x8_w4, b),
                                                 c, 0, 0, 0);
}

// e8m0 byte (1..254) -> the f32 2^(byte - 127)
__device__ __forceinline__ float e8m0_to_f32(uint32_t byte) { return __uint_as_float(byte << 23); }

// the eight e2m1 codes of one 32-bit word (k ascending from the low nibble) x scale -> 8 bf16
__device__ __forceinline__ u16x8 dequant8_fp4(uint32_t word, float scale) {
  const uint32_t a = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 0));
  const uint32_t b = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 1));
  const uint32_t c = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 2));
  const uint32_t d = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(word, scale, 3));
  return __builtin_bit_cast(u16x8, u32x4_w4{a, b, c, d});
}

// Loads of a batch in flight per lane: 5 * NC + 16 * MB registers per chunk (codes, the scale
// word, the X fragments).  Four chunks per batch; two for the widest variant (52 per chunk).
// Four against two everywhere, default groups, two builds alternating in one process: 70B gate/up 1 / 8
// rows 61.7 / 82.7 against 64.5 / 87.9 us, 70B down 38.1 / 44.3 against 41.5 / 46.2, 8B down 1 row 13.0
// against 14.8; level within 4 % on 70B o and 8B qkv (profiles/mxfp4/README.md).
template <int MB, int NC>
constexpr int w4_unroll() {
  return 5 * NC + 16 * MB > 48 ? 2 : 4;
}

// MB: 16-token blocks (1 or 2); X rows >= M are clamped to M - 1 and discarded.
// NW waves per workgroup split K into NW contiguous parts of whole 128-k chunks.
// NC: 16-channel groups per wave (1, 2 or 4).  Every workgroup reads its waves' K parts of X once:
// 2 * M bytes per k against 8 * NC weight bytes, so the X traffic per streamed weight byte falls
// with NC (the X fragments of a chunk feed every channel group's MFMAs) while the grid shrinks.
template <int MB, int NW, int NC>
__global__ void __launch_bounds__(64 * NW) w4a16_gemm_kernel(const uint16_t* __restrict__ X, int64_t ldx,
                                                             const uint8_t* __restrict__ Q,
                                                             const uint8_t* __restrict__ S, uint16_t* __restrict__ Y,
                                                             int64_t ldy, int M, int N, int K) {
  __shared__ f32x4 red[NW][NC][MB][64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16 * NC;
  const int kq = K / NW;  // this wave's K part
  const uint8_t* qrow[NC];   // codes of k = w * kq + 32g .. : byte (w * kq + 32g) / 2 of the channel's row
  const uint8_t* srow[NC];   // the scale word of the wave's first chunk
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int64_t n = n0 + 16 * j + c;
    qrow[j] = Q + n * (K / 2) + (w * kq) / 2 + 16 * g;
    srow[j] = S + n * (K / 32) + (w * kq) / 32;
  }
  const uint16_t* xr[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) xr[mb] = X + (int64_t)min(mb * 16 + c, M - 1) * ldx + (int64_t)w * kq + 32 * g;
  // (Masking the X loads of token columns >= M off instead of clamping their row was measured 10 - 25 %
  // slower at 1 .. 16 rows on every projection shape, e.g. 70B gate/up at 1 row 62 -> 79 us: the compiler
  // then keeps whole batches of loads live, 72 -> 112 VGPRs, and the lost occupancy costs more.)

  f32x4 acc[NC][MB];
#pragma unroll
  for (int j = 0; j < NC; ++j)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) acc[j][mb] = f32x4{0.f, 0.f, 0.f, 0.f};
  // one 128-k chunk: 32 codes per channel group and 4 x 8 activations per lane, four MFMA k-steps
  // per (group, token block)
  auto step = [&](const u32x4_w4 (&q)[NC], const uint32_t (&sw)[NC], const u16x8 (&b)[MB][4]) {
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const float sc = e8m0_to_f32((sw[j] >> (8 * g)) & 0xFFu);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const u16x8 a = dequant8_fp4(q[j][s], sc);  // k = 32g + 8s + 0..7
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) acc[j][mb] = mfma16_w4(a, b[mb][s], acc[j][mb]);
      }
    }
  };
  auto load = [&](int ch, u32x4_w4 (&q)[NC], uint32_t (&sw)[NC], u16x8 (&b)[MB][4]) {
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      q[j] = *reinterpret_cast<const u32x4_w4*>(qrow[j] + ch * 64);
      sw[j] = *reinterpret_cast<const uint32_t*>(srow[j] + ch * 4);
    }
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int s = 0; s < 4; ++s) b[mb][s] = *reinterpret_cast<const u16x8*>(xr[mb] + ch * 128 + 8 * s);
  };
  // batches of U chunks: all of a batch's loads are issued before its first use (a plain loop
  // waits on each).  Whole batches of UNR, then one of UNR / 2 ..., then single chunks.
  auto batch = [&](int ch, auto u_) {
    constexpr int U = decltype(u_)::value;
    u32x4_w4 q[U][NC];
    uint32_t sw[U][NC];
    u16x8 b[U][MB][4];
#pragma unroll
    for (int u = 0; u < U; ++u) load(ch + u, q[u], sw[u], b[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) step(q[u], sw[u], b[u]);
  };
  constexpr int UNR = w4_unroll<MB, NC>();
  const int nch = kq / 128;
  int ch = 0;
  for (; ch + UNR <= nch; ch += UNR) batch(ch, std::integral_constant<int, UNR>{});
  if constexpr (UNR >= 4) {
    if (ch + 2 <= nch) {
      batch(ch, std::integral_constant<int, 2>{});
      ch += 2;
    }
  }
  for (; ch < nch; ++ch) batch(ch, std::integral_constant<int, 1>{});
  // C[row = channel 4g + i][col = token c] per (group, m-block): sum the NW K parts
#pragma unroll
  for (int j = 0; j < NC; ++j)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) red[w][j][mb][lane] = acc[j][mb];
  __syncthreads();
  if (w == 0) {
#pragma unroll
    for (int j = 0; j < NC; ++j) {
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        f32x4 s = red[0][j][mb][lane];
#pragma unroll
        for (int ww = 1; ww < NW; ++ww) s += red[ww][j][mb][lane];
        const int m = mb * 16 + c;
        if (m < M) {
          const int n = n0 + 16 * j + 4 * g;
          u16x4 o;
#pragma unroll
          for (int i = 0; i < 4; ++i) o[i] = f2bf(s[i]);
          *reinterpret_cast<u16x4*>(Y + (int64_t)m * ldy + n) = o;
        }
      }
    }
  }
}

// codes [N, K/2], scales [N, K/32] -> bf16 W [N, K]: one 32-bit code word (8 k, 16 B out) per
// thread and pass; both tensors are contiguous, so word i belongs to scale byte i / 4.
__global__ void __launch_bounds__(256) w4_dequant_kernel(const uint32_t* __restrict__ Q,
                                                         const uint8_t* __restrict__ S, uint16_t* __restrict__ W,
                                                         int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256)
    *reinterpret_cast<u16x8*>(W + i * 8) = dequant8_fp4(Q[i], e8m0_to_f32(S[i >> 2]));
}

template <int MB, int NW>
static void w4_launch_nc(int nc, const W4Launch& L, hipStream_t stream) {
  const uint16_t* x = static_cast<const uint16_t*>(L.x);
  const uint8_t* q = static_cast<const uint8_t*>(L.codes);
  const uint8_t* s = static_cast<const uint8_t*>(L.scales);
  uint16_t* y = static_cast<uint16_t*>(L.y);
  const int M = (int)L.M, N = (int)L.N, K = (int)L.K;
  if (nc == 4) w4a16_gemm_kernel<MB, NW, 4><<<N / 64, 64 * NW, 0, stream>>>(x, L.ldx, q, s, y, L.ldy, M, N, K);
  else if (nc == 2) w4a16_gemm_kernel<MB, NW, 2><<<N / 32, 64 * NW, 0, stream>>>(x, L.ldx, q, s, y, L.ldy, M, N, K);
  else w4a16_gemm_kernel<MB, NW, 1><<<N / 16, 64 * NW, 0, stream>>>(x, L.ldx, q, s, y, L.ldy, M, N, K);
}

}  // namespace mx

using namespace mx;

// Channel groups per wave for a launch.  `force` (MXLLM_W4_NC: 1 / 2 / 4, read per call, the A/B
// switch) is honoured wherever N is whole workgroups of that width and the grid keeps >= 128 of
// them; otherwise, and with force = 0, the default below.
static int w4_groups(int force, int64_t M, int64_t N) {
  auto fits = [&](int nc, int64_t min_wgs) { return N % (16 * nc) == 0 && N / (16 * nc) >= min_wgs; };
  if (force == 1) return 1;
  if ((force == 2 || force == 4) && fits(force, 128)) return force;
  // Defaults from bench/w4_probe.py at the Llama-3.1 70B / 8B projection shapes (us per call, one / two /
  // four groups; full table: profiles/mxfp4/README.md).  More groups cut the X traffic per weight byte but
  // shrink the grid, and a grid much below the 256 CUs loses more than the X traffic costs:
  //   four groups from 8 rows on where they leave >= 160 workgroups
  //     70B qkv (N 10240, 160 WGs)  M 8: 26.5 / 25.9 / 22.9   M 32: 64.6 / 54.1 / 34.8
  //     70B gu  (N 57344)           M 16: 163 / 109 / 102     M 32: 285 / 182 / 128
  //     8B gu   (N 28672)           M 32: 77.1 / 54.5 / 36.6
  //     but 70B o / down (N 8192, 128 WGs)  M 32: 44.8 / 29.0 / 34.3 and 154 / 95.3 / 111
  //   two groups from 4 rows on where they leave >= 192 workgroups
  //     70B down M 4: 45.6 / 40.4 / 65.2   70B gu M 4: 81.8 / 69.0 / 74.0   8B qkv (192 WGs) M 16: 16.1 / 11.6
  //     but 8B down (N 4096, 128 WGs)  M 8: 17.7 / 22.7
  //   up to 3 rows (measured at 1) two groups only on the widest projections (>= 512 workgroups)
  //     70B gu M 1: 67.9 / 60.3 / 69.2   70B qkv M 1: 17.9 / 19.0 / 20.9   8B down M 1: 13.5 / 19.3
  if (M >= 8 && fits(4, 160)) return 4;
  if (fits(2, M >= 4 ? 192 : 512)) return 2;
  return 1;
}

extern "C" int mx_w4a16_gemm(const W4Launch& L, hipStream_t stream) {
  if (L.M <= 0) return 0;
  if (!w4_takes(L)) return -1;
  const char* e = getenv("MXLLM_W4_NC");
  const int nc = w4_groups(e && *e ? atoi(e) : 0, L.M, L.N);
  const int nw = w4_waves(L.K);
  if (L.M <= 16) {
    if (nw == 8) w4_launch_nc<1, 8>(nc, L, stream);
    else w4_launch_nc<1, 4>(nc, L, stream);
  } else {
    if (nw == 8) w4_launch_nc<2, 8>(nc, L, stream);
    else w4_launch_nc<2, 4>(nc, L, stream);
  }
  return (int)hipGetLastError();
}

// codes u8 [N, K/2], scales u8 [N, K/32] (both contiguous) -> bf16 W [N, K].  K % 32 == 0; codes
// 4-B and W 16-B aligned.
extern "C" int mx_w4_dequant(const uint8_t* codes, const uint8_t* scales, uint16_t* w, int64_t N, int64_t K,
                             hipStream_t stream) {
  if (N < 0 || K < 0 || K % 32) return -1;
  const int64_t n8 = N * K / 8;
  if (n8 <= 0) return 0;
  if (!codes || !scales || !w || (uintptr_t)codes % 4 || (uintptr_t)w % 16) return -1;
  const int grid = (int)std::min<int64_t>(8192, (n8 + 255) / 256);
  w4_dequant_kernel<<<grid, 256, 0, stream>>>(reinterpret_cast<const uint32_t*>(codes), scales, w, n8);
  return (int)hipGetLastError();
}
