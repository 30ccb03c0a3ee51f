// Document-masked causal GQA flash attention for packed training sequences, gfx950: forward and split
// backward.  Query i of batch row b sees key j iff doc_start[b, i] <= j <= i (tables: attn_doc_args.h;
// mxllm.ops.doc_bounds builds them), so a packed window attends inside its documents only and the
// kernels skip the key tiles / q tiles that no pair of theirs can need.
//
// The tile bodies are those of attn_fwd.hip (128 query rows per workgroup over 64-key tiles in a 2-slot
// LDS-DMA ring, swapped QK^T so a lane owns one query row) and of the split mode of attn_bwd.hip (a
// 128-key block per workgroup sweeping 64-row q tiles and storing dS^T; a dQ kernel streaming dS^T and
// K tiles), with the same layouts, swizzles, rounding points and log2-domain lse -- copied here, as
// prefill_paged_kv8.hip did, because those kernels sit at the register cap and their schedule depends
// on their source form.  What is new is the table-driven work split:
//  * forward: the tile loop of the q block at q0 starts at key tile doc_start[b, q0] / 64 (a scalar
//    load; earlier tiles are never fetched); a wave works on a tile only if the tile intersects
//    [doc_start of its first row, its last row]; the element mask key < doc_start[row] (one VGPR per
//    lane) is taken, wave-uniformly, only on tiles that start before doc_start of the wave's last row;
//  * key-block kernel: block kb sweeps q tiles from its diagonal to the one holding
//    doc_end[b, last key of the block] - 1; the q rows' doc_start travel with lse / delta through LDS;
//    masked pairs get P = 0 and dS = 0 by selection (exp2(x - lse) of a masked pair can be inf) and the
//    zeros are stored to the dS^T image;
//  * dQ kernel: each 64-row sub-block reads key blocks doc_start[b, its first row] / 128 .. diagonal,
//    exactly pieces the key-block kernel wrote (the invariant: attn_doc_args.h); a piece outside a
//    sub-block's range is fetched from inside it instead and never multiplied.
// No atomics, fixed order: deterministic.  Block order stays by index (q blocks last-first, key blocks
// first-first): with documents that is no longer exactly heaviest-first.
// Every index derived from the tables is clamped (keys to [0, q], q tiles to [diagonal, S)).
#include "attn_doc_args.h"
#include "bindings.h"
#include "common.h"

namespace mx {
namespace {

typedef __bf16 bf16x8_d __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4_d;
typedef int i32x4_d __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const void* gptr_d;
typedef __attribute__((address_space(3))) void* lptr_d;

__device__ __forceinline__ f32x16 mfma32d(const u16x8& a, const u16x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_d, a), __builtin_bit_cast(bf16x8_d, b),
                                                 c, 0, 0, 0);
}
__device__ __forceinline__ u16x4 trdd(const char* p) {
  return __builtin_bit_cast(u16x4, __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_d*)(p)));
}
// 16-B chunk swizzles of the K / V / Q / dO tile rows and of the 128-B dS^T rows (attn_fwd.hip, attn_bwd.hip)
template <int CH>
__device__ __forceinline__ int swzd(int row) {
  return (((row & 3) << 2) | ((row >> 2) & 3)) & (CH - 1);
}
__device__ __forceinline__ int swz8d(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }
__device__ __forceinline__ int clampi(int x, int lo, int hi) { return min(max(x, lo), hi); }

}  // namespace

// ------------------------------------------------------------------------------------------ forward
template <int D>
__global__ void __launch_bounds__(256, 2)
attn_doc_fwd_kernel(const uint16_t* __restrict__ Q, const uint16_t* __restrict__ K, const uint16_t* __restrict__ V,
                    const int* __restrict__ DS, uint16_t* __restrict__ O, float* __restrict__ LSE, int B, int Hq,
                    int Hkv, int S, float sl, int ldo) {
  constexpr int NW = 4;
  constexpr int BM = 32 * NW, BN = 64, CH = D / 8, ROWB = D * 2, KS = D / 16, DB = D / 32;
  constexpr int TILE = BN * ROWB;
  constexpr int LPT = BN * CH / (64 * NW);
  static_assert(LPT >= 1 && BN * CH % (64 * NW) == 0, "K/V tile must split evenly over the waves");
  // ring slot c = K tile, V tile (XOR addressing: 256-B aligned)
  __shared__ __attribute__((aligned(1024))) char smem[2 * 2 * TILE];
  constexpr int VBASE = TILE;
  constexpr auto SOF = [](int c) constexpr { return c * 2 * TILE; };  // byte offset of ring slot c

  const int nqb = (S + BM - 1) / BM;
  const int BH = B * Hq;
  const int bid = xcd_balance(blockIdx.x, gridDim.x, BH, Hq / Hkv);
  const int qb = nqb - 1 - bid / BH;
  const int bh = bid % BH;
  const int b = bh / Hq, h = bh % Hq;
  const int hk = h / (Hq / Hkv);
  const uint16_t* Qp = Q + ((size_t)(b * Hq + h) * S) * D;
  const uint16_t* Kp = K + ((size_t)(b * Hkv + hk) * S) * D;
  const uint16_t* Vp = V + ((size_t)(b * Hkv + hk) * S) * D;
  const int* dsp = DS + (size_t)b * S;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int q0 = qb * BM;
  const int qrow = q0 + 32 * w + r;
  const int qld = min(qrow, S - 1);  // clamped, unconditional loads

  u16x8 qf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) qf[s] = *reinterpret_cast<const u16x8*>(Qp + (size_t)qld * D + 16 * s + 8 * hh);
  // this lane's row: first visible key (one VGPR); the wave's first and last rows' (scalars)
  const int dstart = clampi(dsp[qld], 0, qld);
  const int w_lo = __builtin_amdgcn_readfirstlane(dstart);
  const int w_hi = __builtin_amdgcn_readlane(dstart, 31);

  const int kend = min(S, q0 + BM);
  const int ntiles = (kend + BN - 1) / BN;
  const int kt0 = clampi(dsp[q0] / BN, 0, q0 / BN);  // first key tile of the block: earlier ones are never fetched

  // K/V tiles stream straight into LDS with LDS-DMA through range-checked descriptors: the XOR-swizzled
  // image is produced by permuting each lane's SOURCE chunk; rows past S read as zeros (masked)
  const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc((void*)Kp, 0, S * ROWB, 0x00020000);
  const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc((void*)Vp, 0, S * ROWB, 0x00020000);
  int voff[LPT];
#pragma unroll
  for (int i = 0; i < LPT; ++i) {
    const int seg = w * LPT + i;  // 1 KiB segment of the tile image
    const int byte = seg * 1024 + lane * 16;
    const int row = byte / ROWB, slot = (byte % ROWB) / 16;
    voff[i] = row * ROWB + 16 * (slot ^ swzd<CH>(row));  // logical chunk stored in this slot
  }
  auto glds_piece = [&](int kt, int buf, int i) {
    char* kb = smem + buf * 2 * TILE;
    char* vb = kb + TILE;
    const int seg = w * LPT + i;
    const int off = voff[i] + kt * TILE;  // (through a local: see attn_fwd.hip)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(krs, (lptr_d)(kb + seg * 1024), 16, off, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(vrs, (lptr_d)(vb + seg * 1024), 16, off, 0, 0, 0);
  };

  f32x16 o[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int j = 0; j < 16; ++j) o[d][j] = 0.f;
  // m_i: the (deferred) running max of this row in the log2 domain of the scaled scores; l_i: running
  // sum of exp2(s*sl - m_i).  A wholly masked tile leaves both unchanged: its row max is -inf, so no
  // rescale is triggered for the row (alpha = 1 if another row triggers it) and every p is exp2(-inf) = 0
  float m_i = -1e30f, l_i = 0.f;

  const int g = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
  const uint32_t lds0 = lds_addr(smem);
  uint32_t va_base[DB][2];
#pragma unroll
  for (int db = 0; db < DB; ++db) {
    const int chunk = (db * 32 + 16 * (g & 1) + 4 * tp) >> 3;
    const int rA = 4 * hh + tq, rB = 8 + 4 * hh + tq;
    va_base[db][0] = lds0 + VBASE + rA * ROWB + 16 * (chunk ^ swzd<CH>(rA)) + 8 * (tp & 1);
    va_base[db][1] = lds0 + VBASE + rB * ROWB + 16 * (chunk ^ swzd<CH>(rB)) + 8 * (tp & 1);
  }
  const uint32_t kq_base = lds0 + r * ROWB + 16 * (hh ^ swzd<CH>(r));  // K row r, k step 0 (D = 128 path)
#pragma unroll
  for (int i = 0; i < LPT; ++i) glds_piece(kt0, 0, i);  // the ring's first tile
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): prologue loads and tile-kt0 DMA retired
  __syncthreads();
  const int wq_lo = q0 + 32 * w, wq_hi = wq_lo + 31;

  // One 64-key tile out of ring slot CUR (compile-time).
  auto tile = [&](auto cur_c, int kt) {
    constexpr int CUR = decltype(cur_c)::value;
    constexpr int NXT = CUR ^ 1;
    const int kpf = kt + 1;  // the tile this one prefetches
    const bool more = kpf < ntiles;
    const char* kb = smem + SOF(CUR);
    // the tile intersects [doc_start of the wave's first row, the wave's last row]
    const bool active = (kt * BN <= wq_hi) && (kt * BN + BN - 1 >= w_lo);
    auto pf_piece = [&](int i) { glds_piece(kpf, NXT, i); };
    if (more && !active) {  // an idle wave issues its share of the prefetch at once
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
        // both 32-key chains interleaved; K rows by asm reads one k step ahead (counted waits); the
        // next tile's DMA pieces spread over the k steps
        u16x8 kf2[2][2];
        auto ld = [&](int st, u16x8 (&x)[2]) {
          const uint32_t a = kq_base ^ (uint32_t)(32 * st);
          x[0] = rd128_off(a, SOF(CUR));
          x[1] = rd128_off(a, SOF(CUR) + 32 * ROWB);
        };
        ld(0, kf2[0]);
#pragma unroll
        for (int st = 0; st < KS; ++st) {
          if (st + 1 < KS) ld(st + 1, kf2[(st + 1) & 1]);
          lds_wait_le(st + 1 < KS ? 2 : 0);
          u16x8(&x)[2] = kf2[st & 1];
          pin(x[0]);
          pin(x[1]);
          sacc[0] = mfma32d(x[0], qf[st], sacc[0]);
          sacc[1] = mfma32d(x[1], qf[st], sacc[1]);
          if (more && (st % (KS / LPT)) == 0) pf_piece(st / (KS / LPT));
        }
      } else {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
          const int krow = n * 32 + r;
#pragma unroll
          for (int s = 0; s < KS; ++s) {
            const u16x8 a = *reinterpret_cast<const u16x8*>(kb + krow * ROWB + 16 * ((2 * s + hh) ^ swzd<CH>(krow)));
            sacc[n] = mfma32d(a, qf[s], sacc[n]);
            if (more && n == 0 && (s % (KS / LPT)) == 0) pf_piece(s / (KS / LPT));
          }
        }
      }
      // wave-uniform: the sequence tail, the diagonal, and tiles that start before doc_start of the
      // wave's last row (doc_start is non-decreasing: no earlier row of the wave starts later)
      const bool need_mask = (kt * BN + BN > S) || (kt * BN + BN - 1 > wq_lo) || (kt * BN < w_hi);
      float mp[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      if (need_mask) {  // branch-free select per element: a masked score is -inf, never multiplied by 0
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const int key = kt * BN + n * 32 + (j & 3) + 8 * (j >> 2) + 4 * hh;
            const bool dead = (key >= S) | (key > qrow) | (key < dstart);
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
      float mx = fmaxf(fmaxf(mp[0], mp[1]), fmaxf(mp[2], mp[3]));
      {  // max with the other half-wave (same query row)
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
        mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
      }
      // deferred rescale: only when some row's tile max exceeds its running max by more than 2^8
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
      float lp[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[n][j], sl, nm));
          sacc[n][j] = p;
          lp[j & 3] += p;
        }
      l_i += (lp[0] + lp[1]) + (lp[2] + lp[3]);
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          u16x8 pb;
#pragma unroll
          for (int j = 0; j < 8; ++j) pb[j] = f2bf(sacc[n][8 * s2 + j]);
          // V^T fragments by inline-asm transposed reads behind counted waits (attn_fwd.hip)
          u16x4 fv[DB][2];
#pragma unroll
          for (int db = 0; db < DB; ++db) {
            fv[db][0] = trd_off(va_base[db][0], SOF(CUR) + (32 * n + 16 * s2) * ROWB);
            fv[db][1] = trd_off(va_base[db][1], SOF(CUR) + (32 * n + 16 * s2) * ROWB);
          }
#pragma unroll
          for (int db = 0; db < DB; ++db) {
            lds_wait_le(2 * (DB - 1 - db));
            pin(fv[db][0]);
            pin(fv[db][1]);
            const u16x4 va = fv[db][0], vc = fv[db][1];
            const u16x8 a = u16x8{va[0], va[1], va[2], va[3], vc[0], vc[1], vc[2], vc[3]};
            o[db] = mfma32d(a, pb, o[db]);
          }
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // this wave's DMA for tile kt+1 landed
    __syncthreads();                     // ... and every other wave's; slot CUR free again
  };
  for (int kt = kt0; kt < ntiles; kt += 2) {  // unrolled by the ring depth: static slots
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

// ----------------------------------------------------------------------------------------- backward
// delta[b,h,q] = sum_d dO[b,q,h,d] * O[b,q,h,d]: attn_bwd.hip's delta kernel, unchanged
template <int D>
__global__ void __launch_bounds__(256) attn_doc_delta_kernel(const uint16_t* __restrict__ dO,
                                                             const uint16_t* __restrict__ O,
                                                             float* __restrict__ delta, int B, int S, int Hq,
                                                             int64_t ldo) {
  constexpr int LPR = D / 8;  // lanes per row
  const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LPR;  // over B*S*Hq (token-major order)
  const int sub = threadIdx.x % LPR;
  const bool valid = row < (int64_t)B * S * Hq;
  float s = 0.f;
  if (valid) {
    const u16x8 a = *reinterpret_cast<const u16x8*>(dO + row * D + sub * 8);
    const u16x8 c = *reinterpret_cast<const u16x8*>(O + (row / Hq) * ldo + (row % Hq) * D + sub * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) s += bf2f(a[j]) * bf2f(c[j]);
  }
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (valid && sub == 0) {
    const int h = (int)(row % Hq);
    const int64_t t = row / Hq;
    const int b = (int)(t / S), q = (int)(t % S);
    delta[((int64_t)b * Hq + h) * S + q] = s;
  }
}

// Key-block kernel: workgroup = 4 waves = 128 keys of one q head (32 keys per wave, key on the MFMA
// lane, K / V fragments in registers); it sweeps the 64-row q tiles from its diagonal to the end of the
// last document that holds one of its keys, accumulates the dK / dV partial of its q head and stores
// dS^T (bf16) of every visited tile to the image [BH][S_pad/64][nkb*128 keys][64 q].
template <int D>
__global__ void __launch_bounds__(256, 1)
attn_doc_bwd_kernel(const uint16_t* __restrict__ Q, const uint16_t* __restrict__ K, const uint16_t* __restrict__ V,
                    const uint16_t* __restrict__ dO, const float* __restrict__ LSE, const float* __restrict__ DELTA,
                    const int* __restrict__ DS, const int* __restrict__ DE, uint16_t* __restrict__ dST,
                    float* __restrict__ dKp, float* __restrict__ dVp, int B, int Hq, int Hkv, int S, float sl,
                    float scale, int S_pad) {
  constexpr int BN = 128, BQ = 64, CH = D / 8, ROWB = D * 2, KS = D / 16, DB = D / 32;
  constexpr int QT = BQ * ROWB;    // one Q tile / dO tile [64][D]
  constexpr int SEGS = QT / 1024;  // 1-KiB LDS-DMA segments per tile
  // LDS: 2 x (Q tile, dO tile, lse[64], delta[64], doc_start[64])
  constexpr int BUF = 2 * QT + 3 * BQ * 4;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];

  const int nkb = (S + BN - 1) / BN;
  const int BH = B * Hq;
  const int bid = xcd_balance(blockIdx.x, gridDim.x, BH, Hq / Hkv);
  const int kb = bid / BH;
  const int bh = bid % BH;
  if (kb >= nkb) return;
  const int b = bh / Hq, h = bh % Hq, hk = h / (Hq / Hkv);
  const uint16_t* Qp = Q + (size_t)(b * Hq + h) * S * D;
  const uint16_t* Kp = K + (size_t)(b * Hkv + hk) * S * D;
  const uint16_t* Vp = V + (size_t)(b * Hkv + hk) * S * D;
  const size_t dstride = (size_t)Hq * D;  // token-major row stride of dO
  const uint16_t* dOp = dO + (size_t)b * S * dstride + (size_t)h * D;
  const float* lsep = LSE + (size_t)(b * Hq + h) * S;
  const float* delp = DELTA + (size_t)(b * Hq + h) * S;
  const int* dsp = DS + (size_t)b * S;
  uint16_t* dstp = dST + (size_t)(b * Hq + h) * (nkb * BN) * S_pad;

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int g = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
  const int k0 = kb * BN;
  const int key = k0 + 32 * w + r;  // this lane's key
  const int kld = min(key, S - 1);

  u16x8 kf[KS], vf[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    kf[s] = *reinterpret_cast<const u16x8*>(Kp + (size_t)kld * D + 16 * s + 8 * hh);
    vf[s] = *reinterpret_cast<const u16x8*>(Vp + (size_t)kld * D + 16 * s + 8 * hh);
  }
  f32x16 dk[DB], dv[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int j = 0; j < 16; ++j) { dk[d][j] = 0.f; dv[d][j] = 0.f; }

  // q tiles: the diagonal one .. the one holding the last row that can see a key of this block
  const int qt_lo = k0 / BQ;
  const int qt_hi = clampi((DE[(size_t)b * S + min(k0 + BN - 1, S - 1)] - 1) / BQ, qt_lo, (S - 1) / BQ);
  const int qstart = qt_lo * BQ;
  const int nqt = qt_hi - qt_lo + 1;

  // LDS-DMA of q tile `it` into buffer `buf`: Q / dO rows by range-checked buffer loads (swizzle via
  // source chunk permutation; rows past S read as zeros), lse / delta / doc_start by wave 0
  const int orec = (int)(((size_t)(S - 1) * dstride + D) * 2);
  static_assert(SEGS / 4 <= 4, "at most 4 pieces per wave");
  i32x4_d qoff = {0, 0, 0, 0}, ooff = {0, 0, 0, 0};  // (a vector: a captured int array drops the host stub)
#pragma unroll
  for (int i = 0; i < SEGS / 4; ++i) {
    const int seg = w * (SEGS / 4) + i;
    const int byte = seg * 1024 + lane * 16;
    const int row = byte / ROWB, slot = (byte % ROWB) / 16;
    const int ch = slot ^ swzd<CH>(row);
    qoff[i] = row * ROWB + ch * 16;
    ooff[i] = (int)(row * dstride * 2) + ch * 16;
  }
  auto glds = [&](int it, int buf) {
    char* qt = smem + buf * BUF;
    char* dot = qt + QT;
    char* ld = dot + QT;
    const int q0 = qstart + it * BQ;
    const __amdgpu_buffer_rsrc_t qrs = __builtin_amdgcn_make_buffer_rsrc((void*)Qp, 0, S * ROWB, 0x00020000);
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc((void*)dOp, 0, orec, 0x00020000);
#pragma unroll
    for (int i = 0; i < SEGS / 4; ++i) {
      const int seg = w * (SEGS / 4) + i;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(qrs, (lptr_d)(qt + seg * 1024), 16, qoff[i] + q0 * ROWB, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(ors, (lptr_d)(dot + seg * 1024), 16,
                                               ooff[i] + (int)(q0 * dstride * 2), 0, 0, 0);
    }
    if (w == 0) {
      const int q = min(q0 + lane, S - 1);
      __builtin_amdgcn_global_load_lds((gptr_d)(lsep + q), (lptr_d)(ld), 4, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_d)(delp + q), (lptr_d)(ld + BQ * 4), 4, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_d)(dsp + q), (lptr_d)(ld + 2 * BQ * 4), 4, 0, 0);
    }
  };

  // this wave's dS^T (32 keys x 64 q, bf16) of the previous q tile, stored after the next barrier so the
  // stores drain during a whole tile of compute
  u16x4 dsv[2][4];
  int ds_q0 = -1;
  auto flush_ds = [&]() {
    if (ds_q0 < 0) return;
    uint16_t* rowp = dstp + ((size_t)(ds_q0 / BQ) * (nkb * BN) + (k0 + 32 * w + r)) * BQ;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) *reinterpret_cast<u16x4*>(rowp + 32 * m + 8 * gq + 4 * hh) = dsv[m][gq];
  };

  glds(0, 0);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): prologue loads retired
  __syncthreads();
  for (int it = 0; it < nqt; ++it) {
    const int q0 = qstart + it * BQ;
    const int buf = it & 1;
    const char* qt = smem + buf * BUF;
    const char* dot = qt + QT;
    const float* lse_s = reinterpret_cast<const float*>(dot + QT);
    const float* del_s = lse_s + BQ;
    const int* ds_s = reinterpret_cast<const int*>(del_s + BQ);
    if (it + 1 < nqt) glds(it + 1, buf ^ 1);  // prefetch next tile (its buffer was last read before the barrier)
    flush_ds();
    // wave-uniform: the tails, the diagonal, and tiles whose last row's document starts after the wave's
    // first key (doc_start is non-decreasing: the last row's is the tile's largest)
    const int ds_last = __builtin_amdgcn_readfirstlane(ds_s[BQ - 1]);
    const bool need_mask = (q0 + BQ > S) || (k0 + BN > S) || (k0 + 32 * w + 31 > q0) || (ds_last > k0 + 32 * w);
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      f32x16 sa, dp;
#pragma unroll
      for (int j = 0; j < 16; ++j) { sa[j] = 0.f; dp[j] = 0.f; }
      const int qr = 32 * m + r;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const int o = qr * ROWB + 16 * ((2 * s + hh) ^ swzd<CH>(qr));
        sa = mfma32d(*reinterpret_cast<const u16x8*>(qt + o), kf[s], sa);
        dp = mfma32d(*reinterpret_cast<const u16x8*>(dot + o), vf[s], dp);
      }
      // rows of sa/dp: q = q0 + 32m + (j&3) + 8(j>>2) + 4hh ; column = key (lane)
      f32x4 lv[4], dl[4];
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        lv[gq] = *reinterpret_cast<const f32x4*>(lse_s + 32 * m + 8 * gq + 4 * hh);
        dl[gq] = *reinterpret_cast<const f32x4*>(del_s + 32 * m + 8 * gq + 4 * hh);
      }
      if (need_mask) {  // branch-free selects: a masked pair has P = 0 and dS = 0 whatever exp2 gives
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
          const i32x4_d st = *reinterpret_cast<const i32x4_d*>(ds_s + 32 * m + 8 * gq + 4 * hh);
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) {
            const int j = 4 * gq + jj;
            const int q = q0 + 32 * m + jj + 8 * gq + 4 * hh;
            const bool dead = (key >= S) | (q >= S) | (key > q) | (key < st[jj]);
            const float p = __builtin_amdgcn_exp2f(sa[j] * sl - lv[gq][jj]);
            sa[j] = dead ? 0.f : p;
            dp[j] = dead ? 0.f : p * (dp[j] - dl[gq][jj]);  // dS
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float p = __builtin_amdgcn_exp2f(sa[j] * sl - lv[j >> 2][j & 3]);
          sa[j] = p;
          dp[j] = p * (dp[j] - dl[j >> 2][j & 3]);
        }
      }
      // dV^T += dO^T P ; dK^T += Q^T dS   (k index = q rows of this m-subtile)
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        u16x8 pb, sb;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          pb[j] = f2bf(sa[8 * s2 + j]);
          sb[j] = f2bf(dp[8 * s2 + j]);
        }
        const int rb = 32 * m + 16 * s2 + 4 * hh;
        const int rowA = rb + tq, rowB = rb + 8 + tq;
#pragma unroll
        for (int db = 0; db < DB; ++db) {
          const int chunk = (db * 32 + 16 * (g & 1) + 4 * tp) >> 3;
          const int oA = rowA * ROWB + 16 * (chunk ^ swzd<CH>(rowA)) + 8 * (tp & 1);
          const int oB = rowB * ROWB + 16 * (chunk ^ swzd<CH>(rowB)) + 8 * (tp & 1);
          const u16x4 a0 = trdd(dot + oA), a1 = trdd(dot + oB);
          dv[db] = mfma32d(u16x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]}, pb, dv[db]);
          const u16x4 b0 = trdd(qt + oA), b1 = trdd(qt + oB);
          dk[db] = mfma32d(u16x8{b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]}, sb, dk[db]);
        }
      }
#pragma unroll
      for (int gq = 0; gq < 4; ++gq)
        dsv[m][gq] = u16x4{f2bf(dp[4 * gq]), f2bf(dp[4 * gq + 1]), f2bf(dp[4 * gq + 2]), f2bf(dp[4 * gq + 3])};
    }
    ds_q0 = q0;
    __syncthreads();  // this tile's Q/dO buffer consumed; next tile's DMA landed
  }
  flush_ds();
  // per-q-head dK/dV partials: C rows = d, col = key (lane)
  if (key < S) {
    float* dkq = dKp + ((size_t)(b * Hq + h) * S + key) * D;
    float* dvq = dVp + ((size_t)(b * Hq + h) * S + key) * D;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int gq = 0; gq < 4; ++gq) {
        const int d = db * 32 + 8 * gq + 4 * hh;
        *reinterpret_cast<f32x4*>(dkq + d) =
            f32x4{dk[db][4 * gq] * scale, dk[db][4 * gq + 1] * scale, dk[db][4 * gq + 2] * scale,
                  dk[db][4 * gq + 3] * scale};
        *reinterpret_cast<f32x4*>(dvq + d) = f32x4{dv[db][4 * gq], dv[db][4 * gq + 1], dv[db][4 * gq + 2],
                                                  dv[db][4 * gq + 3]};
      }
  }
}

// dQ kernel: one workgroup per (QB x 64 q rows, q head), 4 waves per 64-row sub-block, all sharing each
// streamed 64-key K tile: dQ[q][:] = scale * sum over key tiles of dS[64 x 64] . K[64 x D], dS^T and K
// tiles through LDS by LDS-DMA in an NSTAGE ring (counted vmcnt waits + bare s_barrier), inline-asm
// tr-reads for both MFMA operands, f32 accumulators in registers, one plain store.  Sub-block j (q tile
// t_j) owns the key tiles lo_j = 2 (doc_start[b, 64 t_j] / 128) .. t_j; the workgroup streams tiles
// lo_0 .. t_last, a sub-block multiplies only inside its range, and its dS^T piece of a tile outside the
// range is fetched from the nearest tile inside it (written, by the invariant of attn_doc_args.h).
template <int D, int QB>
__global__ void __launch_bounds__(256 * QB, 1)
attn_doc_dq_kernel(const uint16_t* __restrict__ dST, const uint16_t* __restrict__ K, const int* __restrict__ DS,
                   float* __restrict__ dQ, int B, int Hq, int Hkv, int S, int S_pad, int Sk_pad, float scale) {
  constexpr int BK = 64, BQ = 64, CH = D / 8, ROWB = D * 2, DB = D / 32;
  constexpr int DSROWB = BQ * 2;  // dS^T image row: 64 q = 128 B
  constexpr int KT = BK * ROWB;   // K tile [64][D]
  constexpr int DT = BK * DSROWB; // one dS^T tile [64 keys][64 q]
  constexpr int BUF = KT + QB * DT;
  constexpr int NSTAGE = QB == 2 ? 4 : 3;
  constexpr int NT = (2 * DB + 3) / 4;
  constexpr int KSEG = KT / 1024, DSEG = DT / 1024;  // 1-KiB LDS-DMA segments
  constexpr int NW = 4 * QB;                         // waves
  constexpr int PER_WAVE = (KSEG + QB * DSEG) / NW;  // DMA instructions per wave per stage
  static_assert((KSEG + QB * DSEG) % NW == 0, "stage must split evenly over the waves");
  static_assert(PER_WAVE <= 4, "piece ranges live in one 4-vector; vmcnt immediate");
  __shared__ __attribute__((aligned(16))) char smem[NSTAGE * BUF];

  const int nqb = (S + BQ * QB - 1) / (BQ * QB);
  const int BH = B * Hq;
  const int bid = xcd_balance(blockIdx.x, gridDim.x, BH, Hq / Hkv);
  const int qb = nqb - 1 - bid / BH;
  const int bh = bid % BH;
  const int b = bh / Hq, h = bh % Hq, hk = h / (Hq / Hkv);
  const int q0 = qb * BQ * QB;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int sub = w / 4, wl = w % 4;  // 64-row sub-block of this wave, wave index within it
  const int r = lane & 31, hh = lane >> 5;
  const int g = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
  const uint16_t* dsp = dST + (size_t)bh * Sk_pad * S_pad;
  const uint16_t* Kp = K + (size_t)(b * Hkv + hk) * S * D;
  const int* dtab = DS + (size_t)b * S;
  const int qt_max = S_pad / BQ - 1;  // the last q tile of the image (its first row is < S)
  // q tile of sub-block j (a tail sub-block past S_pad re-reads the last tile: its rows are not stored)
  // and the first 64-key tile of its range
  auto sub_qt = [&](int j) { return min(q0 / BQ + j, qt_max); };
  auto sub_lo = [&](int j) {
    const int t = sub_qt(j);
    return 2 * clampi(dtab[t * BQ] / 128, 0, t / 2);
  };
  const int it_lo = sub_lo(0), it_hi = sub_qt(QB - 1);  // the key tiles this workgroup streams
  const int nkt = it_hi - it_lo + 1;
  const int my_lo = sub_lo(sub), my_hi = sub_qt(sub);   // ... and this wave multiplies
  const int qsub0 = q0 + BQ * sub;

  // this wave's DMA pieces of a stage: K tile segments, or dS^T segments of sub-block jt with its range
  i32x4_d p_lo = {0, 0, 0, 0}, p_hi = {0, 0, 0, 0}, p_qt = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < PER_WAVE; ++i) {
    const int seg = w * PER_WAVE + i;
    const int jt = seg >= KSEG ? (seg - KSEG) / DSEG : 0;
    p_lo[i] = sub_lo(jt), p_hi[i] = sub_qt(jt), p_qt[i] = sub_qt(jt);
  }
  auto glds = [&](int n) {  // stage n: key tile it_lo + n
    char* kt = smem + (n % NSTAGE) * BUF;
    const int it = it_lo + n;
#pragma unroll
    for (int i = 0; i < PER_WAVE; ++i) {
      const int seg = w * PER_WAVE + i;
      if (seg < KSEG) {
        const int byte = seg * 1024 + lane * 16;
        const int row = byte / ROWB, slot = (byte % ROWB) / 16;
        const int ch = slot ^ swzd<CH>(row);
        const int kk = min(it * BK + row, S - 1);
        __builtin_amdgcn_global_load_lds((gptr_d)(Kp + (size_t)kk * D + ch * 8), (lptr_d)(kt + seg * 1024), 16, 0,
                                         0);
      } else {
        const int sg = seg - KSEG;  // over QB dS^T tiles
        const int jt = sg / DSEG, sgl = sg % DSEG;
        const int byte = sgl * 1024 + lane * 16;
        const int row = byte / DSROWB, slot = (byte % DSROWB) / 16;
        const int ch = slot ^ swz8d(row);
        const int itc = clampi(it, p_lo[i], p_hi[i]);  // never a piece nobody wrote
        __builtin_amdgcn_global_load_lds((gptr_d)(dsp + ((size_t)p_qt[i] * Sk_pad + itc * BK + row) * BQ + ch * 8),
                                         (lptr_d)(kt + KT + jt * DT + sgl * 1024), 16, 0, 0);
      }
    }
  };

  f32x16 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[t][j] = 0.f;
  const uint32_t lds0 = lds_addr(smem);
  uint32_t aA[NT], aB[NT], bA[NT], bB[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int tile = min(wl + 4 * t, 2 * DB - 1);
    const int m = tile / DB, db = tile % DB;
    const int rA0 = 4 * hh + tq, rB0 = rA0 + 8;
    const int qchunk = (32 * m + 16 * (g & 1) + 4 * tp) >> 3;
    const int dchunk = (db * 32 + 16 * (g & 1) + 4 * tp) >> 3;
    aA[t] = KT + sub * DT + rA0 * DSROWB + 16 * (qchunk ^ swz8d(rA0)) + 8 * (tp & 1);
    aB[t] = KT + sub * DT + rB0 * DSROWB + 16 * (qchunk ^ swz8d(rB0)) + 8 * (tp & 1);
    bA[t] = rA0 * ROWB + 16 * (dchunk ^ swzd<CH>(rA0)) + 8 * (tp & 1);
    bB[t] = rB0 * ROWB + 16 * (dchunk ^ swzd<CH>(rB0)) + 8 * (tp & 1);
  }

#pragma unroll
  for (int p = 0; p < NSTAGE - 1; ++p)
    if (p < nkt) glds(p);
  for (int n = 0; n < nkt; ++n) {
    // this wave's DMA for stage n retired (up to NSTAGE-2 later stages may stay in flight), then every wave's
    const int ahead = min(NSTAGE - 2, nkt - 1 - n);
    if (ahead >= 2) __builtin_amdgcn_s_waitcnt(0x0F70 | ((2 * PER_WAVE) & 0xF) | (((2 * PER_WAVE) >> 4) << 14));
    else if (ahead == 1) __builtin_amdgcn_s_waitcnt(0x0F70 | (PER_WAVE & 0xF) | ((PER_WAVE >> 4) << 14));
    else __builtin_amdgcn_s_waitcnt(0x0F70);
    __builtin_amdgcn_s_barrier();  // also: every wave finished stage n-1, whose buffer is refilled below
    if (n + NSTAGE - 1 < nkt) glds(n + NSTAGE - 1);
    const int it = it_lo + n;
    if (it >= my_lo && it <= my_hi) {
      const uint32_t sb = lds0 + (uint32_t)((n % NSTAGE) * BUF);
      if constexpr (NT == 2 && DB == 4) {
        // D = 128: this wave's two tiles are (m = 0, db = wl) and (m = 1, db = wl): one set of K
        // fragments feeds both
        u16x4 fa[2][4][2], fb[4][2];
#define MX_DQ_READ2(S)                                \
  fb[S][0] = trd_asm<S * 16 * ROWB>(sb + bA[0]);      \
  fb[S][1] = trd_asm<S * 16 * ROWB>(sb + bB[0]);      \
  fa[0][S][0] = trd_asm<S * 16 * DSROWB>(sb + aA[0]); \
  fa[0][S][1] = trd_asm<S * 16 * DSROWB>(sb + aB[0]); \
  fa[1][S][0] = trd_asm<S * 16 * DSROWB>(sb + aA[1]); \
  fa[1][S][1] = trd_asm<S * 16 * DSROWB>(sb + aB[1]);
        MX_DQ_READ2(0) MX_DQ_READ2(1) MX_DQ_READ2(2) MX_DQ_READ2(3)
#undef MX_DQ_READ2
        lds_wait_le(12);  // k steps 0 and 1 landed (steps 2 and 3 still in flight)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          pin(fb[s2][0]); pin(fb[s2][1]);
          pin(fa[0][s2][0]); pin(fa[0][s2][1]); pin(fa[1][s2][0]); pin(fa[1][s2][1]);
        }
#pragma unroll
        for (int s2 = 0; s2 < BK / 16; ++s2) {
          if (s2 == 2) {
            lds_wait();
#pragma unroll
            for (int x = 2; x < 4; ++x) {
              pin(fb[x][0]); pin(fb[x][1]);
              pin(fa[0][x][0]); pin(fa[0][x][1]); pin(fa[1][x][0]); pin(fa[1][x][1]);
            }
          }
          const u16x4 b0 = fb[s2][0], b1 = fb[s2][1];
          const u16x8 bf = u16x8{b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const u16x4 a0 = fa[t][s2][0], a1 = fa[t][s2][1];
            acc[t] = mfma32d(u16x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]}, bf, acc[t]);
          }
        }
      } else {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          if (wl + 4 * t < 2 * DB) {
            u16x4 fa[4][2], fb[4][2];
#define MX_DQ_READ(S)                              \
  fa[S][0] = trd_asm<S * 16 * DSROWB>(sb + aA[t]); \
  fa[S][1] = trd_asm<S * 16 * DSROWB>(sb + aB[t]); \
  fb[S][0] = trd_asm<S * 16 * ROWB>(sb + bA[t]);   \
  fb[S][1] = trd_asm<S * 16 * ROWB>(sb + bB[t]);
            MX_DQ_READ(0) MX_DQ_READ(1) MX_DQ_READ(2) MX_DQ_READ(3)
#undef MX_DQ_READ
            lds_wait();
#pragma unroll
            for (int s2 = 0; s2 < 4; ++s2) {
              pin(fa[s2][0]); pin(fa[s2][1]); pin(fb[s2][0]); pin(fb[s2][1]);
            }
#pragma unroll
            for (int s2 = 0; s2 < BK / 16; ++s2) {
              const u16x4 a0 = fa[s2][0], a1 = fa[s2][1], b0 = fb[s2][0], b1 = fb[s2][1];
              acc[t] = mfma32d(u16x8{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]},
                               u16x8{b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]}, acc[t]);
            }
          }
        }
      }
    }
  }
  // C layout: row = qsub0 + 32m + (j&3) + 8(j>>2) + 4hh, col = db*32 + r
  float* dqp = dQ + (size_t)bh * S * D;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int tile = wl + 4 * t;
    if (tile < 2 * DB) {
      const int m = tile / DB, db = tile % DB;
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int q = qsub0 + 32 * m + (j & 3) + 8 * (j >> 2) + 4 * hh;
        if (q < S) dqp[(size_t)q * D + db * 32 + r] = acc[t][j] * scale;
      }
    }
  }
}

}  // namespace mx

using namespace mx;

// Operands and their rules: mx::AdLaunch / mx::ad_takes (attn_doc_args.h).  A refusal launches nothing.
extern "C" int mx_attn_doc(const AdLaunch& L, float scale, hipStream_t stream) {
  if (!ad_takes(L)) return -1;
  if (ad_empty(L)) return 0;
  const uint16_t *q = (const uint16_t*)L.q, *k = (const uint16_t*)L.k, *v = (const uint16_t*)L.v;
  const int *ds = (const int*)L.doc_start, *de = (const int*)L.doc_end;
  const int B = (int)L.B, Hq = (int)L.Hq, Hkv = (int)L.Hkv, S = (int)L.S, D = (int)L.D;
  const float sl = scale * 1.4426950408889634f;
  if (!L.bwd) {
    uint16_t* o = (uint16_t*)L.o;
    float* lse = (float*)L.lse;
    const int grid = ((S + 127) / 128) * B * Hq, ldo = (int)L.ldo;
    if (D == 128) attn_doc_fwd_kernel<128><<<grid, 256, 0, stream>>>(q, k, v, ds, o, lse, B, Hq, Hkv, S, sl, ldo);
    else if (D == 64) attn_doc_fwd_kernel<64><<<grid, 256, 0, stream>>>(q, k, v, ds, o, lse, B, Hq, Hkv, S, sl, ldo);
    else attn_doc_fwd_kernel<32><<<grid, 256, 0, stream>>>(q, k, v, ds, o, lse, B, Hq, Hkv, S, sl, ldo);
    return (int)hipGetLastError();
  }
  const uint16_t *o = (const uint16_t*)L.o, *dout = (const uint16_t*)L.dout;
  const float* lse = (const float*)L.lse;
  float *delta = (float*)L.delta, *dq = (float*)L.dq, *dkp = (float*)L.dkp, *dvp = (float*)L.dvp;
  uint16_t* dst = (uint16_t*)L.work;
  const int64_t dthreads = (int64_t)B * S * Hq * (D / 8);
  const unsigned dgrid = (unsigned)((dthreads + 255) / 256);
  const int nkb = (int)ab_key_blocks(S), S_pad = (int)ab_s_pad(S);
  const int grid = nkb * B * Hq;
#define MX_DOC_BWD(DD, QB)                                                                                         \
  do {                                                                                                             \
    attn_doc_delta_kernel<DD><<<dgrid, 256, 0, stream>>>(dout, o, delta, B, S, Hq, L.ldo);                         \
    attn_doc_bwd_kernel<DD><<<grid, 256, 0, stream>>>(q, k, v, dout, lse, delta, ds, de, dst, dkp, dvp, B, Hq, Hkv, \
                                                      S, sl, scale, S_pad);                                        \
    const int qgrid = ((S + 64 * QB - 1) / (64 * QB)) * B * Hq;                                                    \
    attn_doc_dq_kernel<DD, QB><<<qgrid, 256 * QB, 0, stream>>>(dst, k, ds, dq, B, Hq, Hkv, S, S_pad, nkb * 128,    \
                                                               scale);                                             \
  } while (0)
  // 64 QB q rows per dQ workgroup: 256 at D = 128, 128 at 64, 64 at 32 (attn_bwd.hip)
  if (D == 128) MX_DOC_BWD(128, 4);
  else if (D == 64) MX_DOC_BWD(64, 2);
  else MX_DOC_BWD(32, 1);
#undef MX_DOC_BWD
  return (int)hipGetLastError();
}
