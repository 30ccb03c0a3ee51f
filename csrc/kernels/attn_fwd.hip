// Causal GQA flash-attention forward for gfx950 (SURVEY §2.4 K7 fwd, K13).
//
// Layouts: q [B,Hq,S,D], k/v [B,Hkv,Sk,D] bf16 head-major (written by
// rope_split), o token-major [B,S,Hq,D] (feeds the Wo GEMM directly),
// lse [B,Hq,S] f32 in the log2 domain of the scaled scores.
//
// Structure (CDNA HIP guide App. B "Fused attention prefill"):
//  * workgroup = 4 waves = 128 query rows (256 threads), KV tile = 64 keys;
//  * "swapped" QK^T: S^T = K . Q^T with v_mfma_f32_32x32x16_bf16, so each lane
//    owns one query column and the tile's keys sit in its 16+16 accumulator
//    registers -> row max / row sum are in-register (+1 cross-half shuffle);
//  * the f32 S^T accumulator, converted pairwise to bf16, IS the B operand of
//    O^T += V^T . P^T (guide §3 "accumulator tile as the next MFMA's operand");
//  * V^T fragments come from the row-major V tile via ds_read_b64_tr_b16 (T10);
//  * K/V tiles live in LDS as 16-B-chunk XOR-swizzled images
//    (chunk ^ ((row&3)<<2 | (row>>2)&3)): conflict-free for both the
//    ds_read_b128 row reads of K and the transposed reads of V;
//  * K/V tiles in a 2-slot LDS ring filled by LDS-DMA (tile t+1 issued during
//    tile t's QK^T steps); V^T read with inline-asm tr-reads so hipcc does not
//    drain the in-flight DMA before them; tile loop unrolled by two so every LDS
//    address is a per-lane base + immediate;
//  * softmax: raw-score row max, scale folded into the exp2 argument (one FMA per
//    element), cross-half max/sum by v_permlane32_swap, deferred O rescale
//    (only when a row max grows by > 2^8: guide T13);
//  * causal blocks scheduled heaviest-first, XCD-aware block remap so the
//    q-heads sharing one KV head run on the same XCD (shared L2).
#include <cstdlib>

#include "bindings.h"
#include "common.h"

namespace mx {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));

template <int CH>
__device__ __forceinline__ int swz(int row) {
  return (((row & 3) << 2) | ((row >> 2) & 3)) & (CH - 1);
}

__device__ __forceinline__ f32x16 mfma32(const u16x8& a, const u16x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b),
                                                 c, 0, 0, 0);
}

// One workgroup = 4 waves = 128 query rows sharing every streamed K/V tile (2 waves per SIMD from
// two workgroups), K/V tiles in a 2-slot ring: one tile of DMA in flight ahead of the one consumed.
// (8-wave workgroups, deeper and split rings, a software-pipelined and a ping-pong variant all
// measured the same or slower: archive/experiments/README.md.)
template <int D, bool CAUSAL>
__global__ void __launch_bounds__(256, 2)
attn_fwd_kernel(const uint16_t* __restrict__ Q, const uint16_t* __restrict__ K, const uint16_t* __restrict__ V,
                uint16_t* __restrict__ O, float* __restrict__ LSE, int B, int Hq, int Hkv, int S, int Sk,
                int causal_off, float sl, int ldo, int flags) {
  constexpr int NW = 4;
  constexpr int BM = 32 * NW, BN = 64, CH = D / 8, ROWB = D * 2, KS = D / 16, DB = D / 32;
  constexpr int TILE = BN * ROWB;
  constexpr int LPT = BN * CH / (64 * NW);
  static_assert(LPT >= 1 && BN * CH % (64 * NW) == 0, "K/V tile must split evenly over the waves");
  // ring slot c = K tile, V tile (XOR addressing: 256-B aligned)
  __shared__ __attribute__((aligned(1024))) char smem[2 * 2 * TILE];
  // byte offsets of K ring slot c (from smem) and of V ring slot c (from smem + VBASE): the LDS read
  // bases carry the region start, so every slot offset stays a ds_read immediate (< 64 KiB).
  // (Two functions, as written: the D = 32 kernel's code depends on this form.)
  constexpr int VBASE = TILE;
  constexpr auto KOF = [](int c) constexpr { return c * 2 * TILE; };
  constexpr auto VOF = [](int c) constexpr { return c * 2 * TILE; };

  const int nqb = (S + BM - 1) / BM;
  const int BH = B * Hq;
  const int bid = xcd_balance(blockIdx.x, gridDim.x, BH, Hq / Hkv);
  const int qb = nqb - 1 - bid / BH;
  const int bh = bid % BH;
  const int b = bh / Hq, h = bh % Hq;
  const int hk = h / (Hq / Hkv);
  const uint16_t* Qp = Q + ((size_t)(b * Hq + h) * S) * D;
  const uint16_t* Kp = K + ((size_t)(b * Hkv + hk) * Sk) * D;
  const uint16_t* Vp = V + ((size_t)(b * Hkv + hk) * Sk) * D;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably wave-uniform (no divergent branches)
  const int r = lane & 31, hh = lane >> 5;
  const int q0 = qb * BM;
  const int qrow = q0 + 32 * w + r;
  const int qld = min(qrow, S - 1);  // clamped, unconditional loads: no phi -> no early vmcnt(0)

  u16x8 qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) qf[s] = *reinterpret_cast<const u16x8*>(Qp + (size_t)qld * D + 16 * s + 8 * hh);

  int kend = Sk;
  if (CAUSAL) kend = min(Sk, q0 + BM + causal_off);
  const int ntiles = kend > 0 ? (kend + BN - 1) / BN : 0;

  // K/V tiles stream straight into LDS with LDS-DMA (global_load_lds_dwordx4):
  // one wave instruction writes 1 KiB lane-linearly, so the XOR-swizzled image
  // is produced by permuting each lane's SOURCE chunk (guide rule 21) and no
  // VGPRs are spent on staging (the kernel sits at the 256-VGPR cap).
  typedef __attribute__((address_space(1))) const void* gptr_t;
  typedef __attribute__((address_space(3))) void* lptr_t;
  // buffer_load ... lds through range-checked descriptors: the per-lane source offset of each
  // piece is loop-invariant (one VALU add for the tile step), rows past Sk read as zeros (masked)
  const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc((void*)Kp, 0, Sk * ROWB, 0x00020000);
  const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc((void*)Vp, 0, Sk * ROWB, 0x00020000);
  int voff[LPT];
#pragma unroll
  for (int i = 0; i < LPT; ++i) {
    const int seg = w * LPT + i;            // 1 KiB segment of the tile image
    const int byte = seg * 1024 + lane * 16;
    const int row = byte / ROWB, slot = (byte % ROWB) / 16;
    voff[i] = row * ROWB + 16 * (slot ^ swz<CH>(row));  // logical chunk stored in this slot
  }
  auto glds_piece = [&](int kt, int buf, int i) {
    char* kb = smem + buf * 2 * TILE;
    char* vb = kb + TILE;
    const int seg = w * LPT + i;
    // (through a local: `voff[i] + ...` written straight into the builtin's argument list makes
    // hipcc's host pass drop the kernel's launch stub -- undefined __device_stub__ at load)
    const int off = voff[i] + kt * TILE;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(krs, (lptr_t)(kb + seg * 1024), 16, off, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(vrs, (lptr_t)(vb + seg * 1024), 16, off, 0, 0, 0);
  };
  auto glds = [&](int kt, int buf) {
#pragma unroll
    for (int i = 0; i < LPT; ++i) glds_piece(kt, buf, i);
  };
  // flags & 1: spread the next tile's DMA over the QK^T k steps (one K + V piece per step pair)
  // instead of one burst at the tile top
  const bool spread = (flags & 1) != 0;

  f32x16 o[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int j = 0; j < 16; ++j) o[d][j] = 0.f;
  // m_i: the (deferred) running max of this row in the log2 domain of the scaled
  // scores; l_i: running sum of exp2(s*sl - m_i)
  float m_i = -1e30f, l_i = 0.f;

  // Loop-invariant LDS byte addresses.  The XOR swizzle of a row depends only on
  // row & 15, so for every (n, s2) k-step and both ring buffers a fragment address
  // is one per-lane base + a compile-time immediate (the tile loop is unrolled by
  // two so the buffer index is static): no VALU address math in the loop.
  const int g = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
  const uint32_t lds0 = lds_addr(smem);
  uint32_t va_base[DB][2];
#pragma unroll
  for (int db = 0; db < DB; ++db) {
    const int chunk = (db * 32 + 16 * (g & 1) + 4 * tp) >> 3;
    const int rA = 4 * hh + tq, rB = 8 + 4 * hh + tq;
    va_base[db][0] = lds0 + VBASE + rA * ROWB + 16 * (chunk ^ swz<CH>(rA)) + 8 * (tp & 1);
    va_base[db][1] = lds0 + VBASE + rB * ROWB + 16 * (chunk ^ swz<CH>(rB)) + 8 * (tp & 1);
  }

  const uint32_t kq_base = lds0 + r * ROWB + 16 * (hh ^ swz<CH>(r));  // K row r, k step 0 (D = 128 path)
#pragma unroll
  for (int t = 0; t < 1; ++t)  // the ring's first tile (as a loop: the schedule of the kernel depends on this form)
    if (t < ntiles) glds(t, t);
  // Retire the prologue's Q loads and tile-0 DMA with a wait the compiler's
  // waitcnt pass can see (otherwise it treats them as possibly pending at the
  // loop header and drains the in-loop prefetch under the QK MFMAs).
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
  __syncthreads();
  const int wq_hi = q0 + 32 * w + 31;

  // One 64-key tile out of ring slot CUR (compile-time).
  auto tile = [&](auto cur_c, int kt) {
    constexpr int CUR = decltype(cur_c)::value;
    constexpr int NXT = CUR ^ 1;  // ring slot of tile kt + 1 (the slot tile kt - 1 used)
    const int kpf = kt + 1;       // the tile this one prefetches
    const bool more = kpf < ntiles;
    const char* kb = smem + KOF(CUR);
    const bool active = !CAUSAL || (kt * BN <= wq_hi + causal_off);
    // DMA piece i of this tile's prefetch: K and V of tile kpf
    auto pf_piece = [&](int i) { glds_piece(kpf, NXT, i); };
    if (more && (!spread || !active)) {  // prefetch one tile ahead
#pragma unroll
      for (int i = 0; i < LPT; ++i) pf_piece(i);
    }
    f32x16 sacc[2];
    if (active) {
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int j = 0; j < 16; ++j) sacc[n][j] = 0.f;
      if constexpr (D == 128) {
        // both 32-key chains interleaved; K rows by asm reads one k step ahead (counted waits).
        // Key rows 32n + r share row & 15 with r, hence the swizzle: k step s is base ^ (32 s),
        // the buffer and the 32-row block n are immediates
        u16x8 kf2[2][2];
        auto ld = [&](int st, u16x8 (&x)[2]) {
          const uint32_t a = kq_base ^ (uint32_t)(32 * st);
          x[0] = rd128_off(a, KOF(CUR));
          x[1] = rd128_off(a, KOF(CUR) + 32 * ROWB);
        };
        ld(0, kf2[0]);
#pragma unroll
        for (int st = 0; st < KS; ++st) {
          if (st + 1 < KS) ld(st + 1, kf2[(st + 1) & 1]);
          lds_wait_le(st + 1 < KS ? 2 : 0);
          u16x8(&x)[2] = kf2[st & 1];
          pin(x[0]);
          pin(x[1]);
          sacc[0] = mfma32(x[0], qf[st], sacc[0]);
          sacc[1] = mfma32(x[1], qf[st], sacc[1]);
          if (spread && more && (st % (KS / LPT)) == 0) pf_piece(st / (KS / LPT));
        }
      } else {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const int krow = n * 32 + r;
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            const u16x8 a = *reinterpret_cast<const u16x8*>(kb + krow * ROWB + 16 * ((2 * s + hh) ^ swz<CH>(krow)));
            sacc[n] = mfma32(a, qf[s], sacc[n]);
            if (spread && more && n == 0 && (s % (KS / LPT)) == 0) pf_piece(s / (KS / LPT));
          }
        }
      }
      // row max of the RAW scores (the scale is folded into the exp2 argument below)
      float mx = -INFINITY;
      const bool need_mask = (kt * BN + BN > Sk) || (CAUSAL && (kt * BN + BN - 1 > q0 + 32 * w + causal_off));
      // 4 independent partial maxima (a 32-long dependent fmax chain otherwise)
      float mp[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      if (need_mask) {  // wave-uniform: diagonal / tail tiles only; branch-free select per element
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const int key = kt * BN + n * 32 + (j & 3) + 8 * (j >> 2) + 4 * hh;
            const bool dead = (key >= Sk) | (CAUSAL & (key > qrow + causal_off));
            const float x = dead ? -INFINITY : sacc[n][j];
            sacc[n][j] = x;
            mp[j & 3] = fmaxf(mp[j & 3], x);
          }
      } else {
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int j = 0; j < 16; ++j) mp[j & 3] = fmaxf(mp[j & 3], sacc[n][j]);
      }
      mx = fmaxf(fmaxf(mp[0], mp[1]), fmaxf(mp[2], mp[3]));
      {  // max with the other half-wave (same query column): one permlane32 swap
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
        mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
      }
      // Deferred rescale (guide T13): O and l are rescaled only when some row's
      // tile max exceeds its running max by more than kThr (log2 units), so
      // probabilities stay <= 2^kThr; the decision is wave-uniform and taken before
      // this tile's P is formed, so everything at the old scale is rescaled once.
      constexpr float kThr = 8.f;
      const float mt = mx * sl;
      if (__any(mt > m_i + kThr)) {
        const float mnew = fmaxf(m_i, mt);
        const float alpha = __builtin_amdgcn_exp2f(m_i - mnew);
        l_i *= alpha;
        m_i = mnew;
#pragma unroll
        for (int d = 0; d < DB; ++d) o[d] *= alpha;
      }
      const float nm = -m_i;
      float lp[4] = {0.f, 0.f, 0.f, 0.f};  // 4 independent partial sums
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[n][j], sl, nm));
          sacc[n][j] = p;
          lp[j & 3] += p;
        }
      l_i += (lp[0] + lp[1]) + (lp[2] + lp[3]);
    }
    if (active) {
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          u16x8 pb;
#pragma unroll
          for (int j = 0; j < 8; ++j) pb[j] = f2bf(sacc[n][8 * s2 + j]);
          // V^T fragments by inline-asm transposed reads (a builtin tr-read makes hipcc
          // drain the next tile's in-flight LDS-DMA here), consumed behind counted waits
          u16x4 fv[DB][2];
#pragma unroll
          for (int db = 0; db < DB; ++db) {
            fv[db][0] = trd_off(va_base[db][0], VOF(CUR) + (32 * n + 16 * s2) * ROWB);
            fv[db][1] = trd_off(va_base[db][1], VOF(CUR) + (32 * n + 16 * s2) * ROWB);
          }
#pragma unroll
          for (int db = 0; db < DB; ++db) {
            lds_wait_le(2 * (DB - 1 - db));
            pin(fv[db][0]);
            pin(fv[db][1]);
            const u16x4 va = fv[db][0], vc = fv[db][1];
            const u16x8 a = u16x8{va[0], va[1], va[2], va[3], vc[0], vc[1], vc[2], vc[3]};
            o[db] = mfma32(a, pb, o[db]);
          }
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // this wave's DMA for tile kt+1 landed
    __syncthreads();                     // ... and every other wave's; slot CUR free again
  };
  for (int kt = 0; kt < ntiles; kt += 2) {  // unrolled by the ring depth: static slots
    tile(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < ntiles) tile(std::integral_constant<int, 1>{}, kt + 1);
  }
  float l_tot;
  {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_i), __float_as_uint(l_i), false, false);
    l_tot = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
  }
  const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
  if (qrow < S) {
    uint16_t* op = O + ((size_t)b * S + qrow) * (size_t)ldo + (size_t)h * D;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int d = db * 32 + 8 * gq + 4 * hh;
        u16x4 v4;
#pragma unroll
        for (int j = 0; j < 4; ++j) v4[j] = f2bf(o[db][4 * gq + j] * inv);
        *reinterpret_cast<u16x4*>(op + d) = v4;
      }
    if (hh == 0) LSE[(size_t)(b * Hq + h) * S + qrow] = m_i + __log2f(l_tot);
  }
}

}  // namespace mx

using namespace mx;

// o: token-major [B, S, Hq*D] rows with row stride ldo (elements, >= Hq*D): the rows may
// be the left part of the LoRA-augmented o-projection input (mxllm/ops/linear.py)
// (operand rules: mx::af_takes, attn_args.h)
extern "C" int mx_attn_fwd(const AfLaunch& L, float scale, hipStream_t stream) {
  if (!af_takes(L)) return -1;
  if (af_empty(L)) return 0;
  const uint16_t *q = (const uint16_t*)L.q, *k = (const uint16_t*)L.k, *v = (const uint16_t*)L.v;
  uint16_t* o = (uint16_t*)L.o;
  float* lse = (float*)L.lse;
  const int B = (int)L.B, Hq = (int)L.Hq, Hkv = (int)L.Hkv, S = (int)L.S, Sk = (int)L.Sk, ldo = (int)L.ldo;
  const int64_t D = L.D;
  const bool causal = L.causal != 0;
  const float sl = scale * 1.4426950408889634f;
  const int off = Sk - S;
  static const int fflags = [] {  // MXLLM_ATTN_FWD_FLAGS (default 1): bit 0 = spread the K/V DMA issue
    const char* e = getenv("MXLLM_ATTN_FWD_FLAGS");   // (B2 0.192 -> 0.186 ms, B16 1.372 -> 1.357 ms)
    return e && *e ? atoi(e) : 1;
  }();
#define FWD(DD, C)                                                                                           \
  attn_fwd_kernel<DD, C><<<((S + 127) / 128) * B * Hq, 256, 0, stream>>>(q, k, v, o, lse, B, Hq, Hkv, S, Sk, \
                                                                         off, sl, ldo, fflags)
  if (D == 128) { if (causal) FWD(128, true); else FWD(128, false); }
  else if (D == 64) { if (causal) FWD(64, true); else FWD(64, false); }
  else { if (causal) FWD(32, true); else FWD(32, false); }
#undef FWD
  return (int)hipGetLastError();
}
