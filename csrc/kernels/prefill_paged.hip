// Causal GQA flash attention of query segments over the paged bf16 KV cache, head_dim 128, gfx950.
//
// A segment is n query rows at positions p0 .. p0 + n - 1 of a cache slot; row t sees keys
// 0 .. p0 + t of that slot, read from the block pools [blocks, Hkv, blk, 128] through the block table.
// The keys of the chunk itself are already in the cache (rope_append ran first).  This is what chunked
// prefill and a prefix-cache hit need: attention from new tokens over rows that sit in the pool.
//
// Layouts: q [T, Hq, 128] token-major (rope_append's output), o [T, ldo] token-major (feeds the Wo
// GEMM), segment table int32 [nseg, 4] = (first q row, n, slot, p0), work table int32 [nwork, 2] =
// (segment, q-block) heaviest first (mx::pp_fill_work).  One workgroup per (work item, q-head).
//
// The tile body is attn_fwd.hip's default kernel, attn_fwd_kernel<128, true, 4>, with the same rounding
// points -- swapped QK^T on v_mfma_f32_32x32x16_bf16, raw-score row max with the scale folded into the
// exp2 argument, P rounded to bf16 as the PV operand, the deferred rescale (threshold 2^8), V^T by
// ds_read_b64_tr_b16, K/V tiles by LDS-DMA with the source-side swizzle into a two-slot ring -- so its
// error model (tests/_parity.py ATTN_O) carries over.  What differs is where a tile comes from:
//  * blk is a multiple of 256, so a 64-key tile lies in one block: its source is
//    pool + ((bt[slot, key / blk] * Hkv + hk) * blk + key % blk) * 128;
//  * tiles are staged in key order, so the block walk is a counter; the id of block j + 1 is loaded when
//    block j is entered (a scalar load one block = at least four tiles ahead of the DMA that needs it)
//    and passes through readfirstlane before it enters the buffer descriptor, so the descriptor is
//    provably wave-uniform and the LDS-DMA needs no waterfall loop;
//  * the descriptor of a block holds num_records = min(blk, p0 + n - block start) * 256 bytes: rows past
//    the segment's end read as zeros.  Stale rows of a recycled block (possibly NaN) never reach an
//    MFMA -- a masked P of 0 times NaN would be NaN;
//  * rows of a partly filled last q-block load clamped inside their own segment and are not stored;
//    output rows outside every segment are not written.  No lse.
#include <type_traits>

#include "bindings.h"
#include "common.h"

namespace mx {

typedef __bf16 pp_bf16x8_t __attribute__((ext_vector_type(8)));

__device__ __forceinline__ int pp_swz(int row) { return (((row & 3) << 2) | ((row >> 2) & 3)) & 15; }

__device__ __forceinline__ f32x16 pp_mfma32(const u16x8& a, const u16x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(pp_bf16x8_t, a),
                                                 __builtin_bit_cast(pp_bf16x8_t, b), c, 0, 0, 0);
}

__device__ __forceinline__ int pp_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__global__ void __launch_bounds__(256, 2)
prefill_paged_kernel(const uint16_t* __restrict__ Q, const uint16_t* __restrict__ KP, const uint16_t* __restrict__ VP,
                     uint16_t* __restrict__ O, const int32_t* __restrict__ bt, const int32_t* __restrict__ segs,
                     const int32_t* __restrict__ work, int Hq, int Hkv, int blocks, int blk, int maxb, float sl,
                     int ldo) {
  constexpr int D = 128, NW = 4, BM = PP_BM, BN = PP_BN, CH = D / 8, ROWB = D * 2, KS = D / 16, DB = D / 32;
  constexpr int TILE = BN * ROWB;            // 16 KiB
  constexpr int LPT = BN * CH / (64 * NW);   // 1 KiB DMA pieces per wave per tile
  static_assert(BM == 32 * NW && LPT == 4, "4 waves x 32 rows, 4 pieces per wave");
  __shared__ __attribute__((aligned(1024))) char smem[4 * TILE];  // ring slot c: K at 2c TILE, V at (2c + 1) TILE
  constexpr int VBASE = TILE;

  const int G = Hq / Hkv;
  const int bid = xcd_balance(blockIdx.x, gridDim.x, Hq, G);
  const int wi = bid / Hq, h = bid % Hq, hk = h / G;
  const int sg = pp_uniform(work[2 * wi]), qb = pp_uniform(work[2 * wi + 1]);
  const int row0 = pp_uniform(segs[4 * sg]), n = pp_uniform(segs[4 * sg + 1]);
  const int slot = pp_uniform(segs[4 * sg + 2]), p0 = pp_uniform(segs[4 * sg + 3]);
  const int Sk = p0 + n;  // keys of the slot this segment may see

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, hh = lane >> 5;
  const int q0 = qb * BM;
  const int qrow = q0 + 32 * w + r;   // row inside the segment; its position is p0 + qrow
  const int qld = min(qrow, n - 1);   // clamped inside the segment: unconditional loads

  u16x8 qf[KS];
  {
    const uint16_t* qp = Q + ((size_t)(row0 + qld) * Hq + h) * D;
#pragma unroll
    for (int s = 0; s < KS; ++s) qf[s] = *reinterpret_cast<const u16x8*>(qp + 16 * s + 8 * hh);
  }

  const int kend = min(Sk, q0 + BM + p0);
  const int ntiles = (kend + BN - 1) / BN;  // >= 1: n > 0

  typedef __attribute__((address_space(3))) void* lptr_t;
  int voff[LPT];
#pragma unroll
  for (int i = 0; i < LPT; ++i) {
    const int byte = (w * LPT + i) * 1024 + lane * 16;
    const int row = byte / ROWB, sl16 = (byte % ROWB) / 16;
    voff[i] = row * ROWB + 16 * (sl16 ^ pp_swz(row));  // logical chunk stored in this LDS slot
  }

  // ---- the block walk.  stage() is called once per tile, in key order, before that tile's DMA pieces.
  const int32_t* btr = bt + (size_t)slot * maxb;
  const int tpb = blk / BN;               // tiles per block
  const int nb = (Sk + blk - 1) / blk;    // blocks of the slot this segment reads
  int t_in = tpb, jb = -1;                // tile inside the block, block index: the first stage() enters block 0
  int bid_nx = btr[0];                    // id of block jb + 1
  const uint16_t* kblk = KP;
  const uint16_t* vblk = VP;
  int nrec = 0, toff = 0;
  auto stage = [&]() {
    if (t_in == tpb) {
      t_in = 0;
      ++jb;
      const int b = min(max(pp_uniform(bid_nx), 0), blocks - 1);  // wave-uniform, inside the pool
      const size_t eoff = ((size_t)b * Hkv + hk) * (size_t)blk * D;
      kblk = KP + eoff;
      vblk = VP + eoff;
      nrec = min(blk, Sk - jb * blk) * ROWB;  // rows past the segment's end read as zeros
      bid_nx = btr[min(jb + 1, nb - 1)];
    }
    toff = t_in * TILE;
    ++t_in;
  };
  // piece i of the staged tile into ring slot buf (the source offset goes through a local: written
  // straight into the builtin's argument list it makes hipcc's host pass drop the launch stub)
  auto glds_piece = [&](int buf, int i) {
    const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc((void*)kblk, 0, nrec, 0x00020000);
    const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc((void*)vblk, 0, nrec, 0x00020000);
    char* kb = smem + buf * 2 * TILE;
    char* vb = kb + TILE;
    const int seg = w * LPT + i;
    const int off = voff[i] + toff;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(krs, (lptr_t)(kb + seg * 1024), 16, off, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(vrs, (lptr_t)(vb + seg * 1024), 16, off, 0, 0, 0);
  };

  f32x16 o[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int j = 0; j < 16; ++j) o[d][j] = 0.f;
  float m_i = -1e30f, l_i = 0.f;  // deferred running max (log2 domain of the scaled scores), running sum

  const int g = lane >> 4, li = lane & 15, tq = li >> 2, tp = li & 3;
  const uint32_t lds0 = lds_addr(smem);
  uint32_t va_base[DB][2];
#pragma unroll
  for (int db = 0; db < DB; ++db) {
    const int chunk = (db * 32 + 16 * (g & 1) + 4 * tp) >> 3;
    const int rA = 4 * hh + tq, rB = 8 + 4 * hh + tq;
    va_base[db][0] = lds0 + VBASE + rA * ROWB + 16 * (chunk ^ pp_swz(rA)) + 8 * (tp & 1);
    va_base[db][1] = lds0 + VBASE + rB * ROWB + 16 * (chunk ^ pp_swz(rB)) + 8 * (tp & 1);
  }
  const uint32_t kq_base = lds0 + r * ROWB + 16 * (hh ^ pp_swz(r));

  stage();
#pragma unroll
  for (int i = 0; i < LPT; ++i) glds_piece(0, i);
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): Q and tile 0, visible to hipcc's waitcnt pass
  __syncthreads();
  const int wq_hi = q0 + 32 * w + 31;

  auto tile = [&](auto cur_c, int kt) {
    constexpr int CUR = decltype(cur_c)::value;
    constexpr int NXT = CUR ^ 1;
    constexpr int KOF = CUR * 2 * TILE;
    const bool more = kt + 1 < ntiles;
    const bool active = kt * BN <= wq_hi + p0;
    if (more) stage();
    if (more && !active) {
#pragma unroll
      for (int i = 0; i < LPT; ++i) glds_piece(NXT, i);
    }
    f32x16 sacc[2];
    if (active) {
#pragma unroll
      for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int j = 0; j < 16; ++j) sacc[nn][j] = 0.f;
      u16x8 kf2[2][2];
      auto ld = [&](int st, u16x8 (&x)[2]) {
        const uint32_t a = kq_base ^ (uint32_t)(32 * st);
        x[0] = rd128_off(a, KOF);
        x[1] = rd128_off(a, KOF + 32 * ROWB);
      };
      ld(0, kf2[0]);
#pragma unroll
      for (int st = 0; st < KS; ++st) {
        if (st + 1 < KS) ld(st + 1, kf2[(st + 1) & 1]);
        lds_wait_le(st + 1 < KS ? 2 : 0);
        u16x8(&x)[2] = kf2[st & 1];
        pin(x[0]);
        pin(x[1]);
        sacc[0] = pp_mfma32(x[0], qf[st], sacc[0]);
        sacc[1] = pp_mfma32(x[1], qf[st], sacc[1]);
        if (more && (st % (KS / LPT)) == 0) glds_piece(NXT, st / (KS / LPT));  // the next tile's DMA, spread
      }
      // row max of the raw scores; tiles on the diagonal or at the segment's end are masked
      const bool need_mask = (kt * BN + BN > Sk) || (kt * BN + BN - 1 > q0 + 32 * w + p0);
      float mp[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      if (need_mask) {
#pragma unroll
        for (int nn = 0; nn < 2; ++nn)
#pragma unroll
          for (int j = 0; j < 16; ++j) {
            const int key = kt * BN + nn * 32 + (j & 3) + 8 * (j >> 2) + 4 * hh;
            const bool dead = (key >= Sk) | (key > qrow + p0);
            const float x = dead ? -INFINITY : sacc[nn][j];
            sacc[nn][j] = x;
            mp[j & 3] = fmaxf(mp[j & 3], x);
          }
      } else {
#pragma unroll
        for (int nn = 0; nn < 2; ++nn)
#pragma unroll
          for (int j = 0; j < 16; ++j) mp[j & 3] = fmaxf(mp[j & 3], sacc[nn][j]);
      }
      float mx = fmaxf(fmaxf(mp[0], mp[1]), fmaxf(mp[2], mp[3]));
      {
        const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mx), __float_as_uint(mx), false, false);
        mx = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
      }
      constexpr float kThr = 8.f;  // deferred rescale: only when a row max grows by more than 2^8
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
      for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[nn][j], sl, nm));
          sacc[nn][j] = p;
          lp[j & 3] += p;
        }
      l_i += (lp[0] + lp[1]) + (lp[2] + lp[3]);
#pragma unroll
      for (int nn = 0; nn < 2; ++nn)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          u16x8 pb;
#pragma unroll
          for (int j = 0; j < 8; ++j) pb[j] = f2bf(sacc[nn][8 * s2 + j]);
          u16x4 fv[DB][2];
#pragma unroll
          for (int db = 0; db < DB; ++db) {
            fv[db][0] = trd_off(va_base[db][0], KOF + (32 * nn + 16 * s2) * ROWB);
            fv[db][1] = trd_off(va_base[db][1], KOF + (32 * nn + 16 * s2) * ROWB);
          }
#pragma unroll
          for (int db = 0; db < DB; ++db) {
            lds_wait_le(2 * (DB - 1 - db));
            pin(fv[db][0]);
            pin(fv[db][1]);
            const u16x4 va = fv[db][0], vc = fv[db][1];
            const u16x8 a = u16x8{va[0], va[1], va[2], va[3], vc[0], vc[1], vc[2], vc[3]};
            o[db] = pp_mfma32(a, pb, o[db]);
          }
        }
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);  // this wave's DMA of tile kt + 1 landed
    __syncthreads();                     // ... and every other wave's; slot CUR is free again
  };
  for (int kt = 0; kt < ntiles; kt += 2) {
    tile(std::integral_constant<int, 0>{}, kt);
    if (kt + 1 < ntiles) tile(std::integral_constant<int, 1>{}, kt + 1);
  }

  float l_tot;
  {
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_i), __float_as_uint(l_i), false, false);
    l_tot = __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
  }
  const float inv = l_tot > 0.f ? 1.f / l_tot : 0.f;
  if (qrow < n) {
    uint16_t* op = O + (size_t)(row0 + qrow) * (size_t)ldo + (size_t)h * D;
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
  }
}

}  // namespace mx

using namespace mx;

extern "C" int mx_prefill_attn_paged(const mx::PpLaunch& L, float scale, hipStream_t stream) {
  if (L.nseg <= 0) return 0;
  if (!pp_takes(L)) return -1;
  const float sl = scale * 1.4426950408889634f;
  prefill_paged_kernel<<<(unsigned)(L.nwork * L.Hq), 256, 0, stream>>>(
      (const uint16_t*)L.q, (const uint16_t*)L.k_pool, (const uint16_t*)L.v_pool, (uint16_t*)L.o, L.bt, L.segs,
      L.work, (int)L.Hq, (int)L.Hkv, (int)L.blocks, (int)L.blk, (int)L.maxb, sl, (int)L.ldo);
  return (int)hipGetLastError();
}
