// Causal GQA flash attention of query segments over the paged fp8 (kv8) KV cache, head_dim 128, gfx950.
//
// prefill_paged.hip over the four kv8 pools: codes [blocks, Hkv, blk, 128] u8 and scales [blocks, Hkv, blk]
// f32 powers of two, for K and for V (format: mxllm/serve/quant.py kv8_quantize, helpers: kv8.h).  Segments,
// the work table, the grid (one workgroup per (work item, q-head), 128 query rows on 4 waves, 64-key tiles)
// and the block walk are that kernel's, and so is the tile body with every rounding point -- swapped QK^T on
// v_mfma_f32_32x32x16_bf16, raw-score row max, P rounded to bf16, the deferred rescale at 2^8, V^T by
// ds_read_b64_tr_b16 out of the two-slot ring of swizzled bf16 K and V images (4 x 16 KiB) -- so its error
// model (tests/_parity.py ATTN_O) carries over.  What differs is how a tile reaches the ring:
//  * no LDS-DMA.  A 64-key tile is 8 KiB of K codes and 8 KiB of V codes: each of the 256 threads loads two
//    16-byte pieces of each (rows pp8_row(tid / 8) and + 32, codes 16 (tid % 8) .. + 15) and the f32 scales of
//    its two rows into registers.  The loads of tile kt + 1 are issued at the top of tile kt, before its
//    QK^T; the K pieces are decoded in the second half of the QK^T k-steps and the V pieces between the PV
//    groups, one pp8_dec8 pair and two 16-byte LDS stores per step, into the positions of ring slot NXT that
//    the DMA of the bf16 kernel fills: row * 256 + 16 * (chunk ^ pp_swz(row)).  Every code is decoded once
//    per workgroup; the tile barrier is unchanged;
//  * BOTH scales are folded in at decode (pp8_dec8(lo, hi, scale) = kv8.h's kv8_dec8(lo, hi, scale): a code
//    times 2^e is exactly a bf16 value), not applied to the score as decode.hip's KvFp8::score does.  The ring then holds exactly the
//    kv8_dequantize'd cache, the tile body needs no per-key multiply in its score loop, and the output is
//    bit for bit prefill_attn_paged's over the dequantised pools;
//  * the lanes of one 16-lane store group hold rows r and r + 4 (pp8_row): pp_swz of the two differs in
//    bit 0, so their even (or odd) chunks fill all 16 slots of a 256-B bank row -- no store conflicts;
//  * rows at or past the segment's end Sk = p0 + n are never loaded, codes or scales: the row index is
//    clamped to Sk - 1, which lies in the same tile.  Such a key is masked (P = 0) and the row it repeats is
//    finite, so stale or NaN rows of a recycled block never reach an MFMA;
//  * no bf16 copy of the cache exists outside LDS.
// Compiled without packed-f32 VALU forms (mxllm/_build.py PER_FILE_HIP_FLAGS).
// Compared and dropped: the same feed decoding with kv8_dec8 (conversion, f32 product, permute) -- the same
// bits, 5 to 8 % slower at every context length (profiles/prefix_cache/README.md): the decode competes with
// the softmax for VALU issue in the waves that feed the MFMAs.
// hipcc --offload-arch=gfx950, compiler metadata: 202 VGPRs, 63 SGPRs, 0 B scratch, no spills, 65536 B LDS
// (prefill_paged_kernel: 182 VGPRs, 0 B scratch, 65536 B LDS) -- two workgroups per CU, as launch_bounds asks.
#include <type_traits>

#include "bindings.h"
#include "common.h"
#include "kv8.h"

namespace mx {

typedef __bf16 pp8_bf16x8_t __attribute__((ext_vector_type(8)));

__device__ __forceinline__ int pp_swz(int row) { return (((row & 3) << 2) | ((row >> 2) & 3)) & 15; }

// row of a tile half (0 .. 31) that 8-lane group a holds: bits 0 and 2 of a swapped
__device__ __forceinline__ int pp8_row(int a) { return (a & ~5) | ((a & 1) << 2) | ((a >> 2) & 1); }

__device__ __forceinline__ f32x16 pp8_mfma32(const u16x8& a, const u16x8& b, const f32x16& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(pp8_bf16x8_t, a),
                                                 __builtin_bit_cast(pp8_bf16x8_t, b), c, 0, 0, 0);
}

// 8 e4m3 codes times sc (a power of two) -> 8 bf16, as kv8_dec8(lo, hi, sc) gives them, in four
// v_cvt_scalef32_pk_bf16_fp8 instead of four conversions, eight products and four permutes: the decode shares
// the VALU with the softmax of the tile body, and that, not the MFMAs, is what bounds this kernel
typedef __bf16 pp8_bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ u16x8 pp8_dec8(uint32_t lo, uint32_t hi, float sc) {
  const pp8_bf16x2_t a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)lo, sc, false);
  const pp8_bf16x2_t b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)lo, sc, true);
  const pp8_bf16x2_t c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)hi, sc, false);
  const pp8_bf16x2_t d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)hi, sc, true);
  return __builtin_bit_cast(u16x8, u32x4{__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b),
                                         __builtin_bit_cast(uint32_t, c), __builtin_bit_cast(uint32_t, d)});
}

__device__ __forceinline__ int pp8_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__global__ void __launch_bounds__(256, 2)
prefill_paged_kv8_kernel(const uint16_t* __restrict__ Q, const uint8_t* __restrict__ KC, const float* __restrict__ KS_,
                         const uint8_t* __restrict__ VC, const float* __restrict__ VS_, uint16_t* __restrict__ O,
                         const int32_t* __restrict__ bt, const int32_t* __restrict__ segs,
                         const int32_t* __restrict__ work, int Hq, int Hkv, int blocks, int blk, int maxb, float sl,
                         int ldo) {
  constexpr int D = 128, NW = 4, BM = PP_BM, BN = PP_BN, ROWB = D * 2, KS = D / 16, DB = D / 32;
  constexpr int TILE = BN * ROWB;  // 16 KiB
  constexpr int NP = 2;            // 16-code pieces of K (and of V) per thread and tile
  static_assert(BM == 32 * NW && BN * D == 256 * NP * 16, "4 waves x 32 rows, 2 pieces per thread");
  __shared__ __attribute__((aligned(1024))) char smem[4 * TILE];  // ring slot c: K at 2c TILE, V at (2c + 1) TILE
  constexpr int VBASE = TILE;

  const int G = Hq / Hkv;
  const int bid = xcd_balance(blockIdx.x, gridDim.x, Hq, G);
  const int wi = bid / Hq, h = bid % Hq, hk = h / G;
  const int sg = pp8_uniform(work[2 * wi]), qb = pp8_uniform(work[2 * wi + 1]);
  const int row0 = pp8_uniform(segs[4 * sg]), n = pp8_uniform(segs[4 * sg + 1]);
  const int slot = pp8_uniform(segs[4 * sg + 2]), p0 = pp8_uniform(segs[4 * sg + 3]);
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

  // this thread's pieces: rows prow and prow + 32 of a tile, codes 16 c16 .. + 15 = bf16 chunks 2 c16, 2 c16 + 1
  const int prow = pp8_row(tid >> 3), c16 = tid & 7;
  int soff[NP][2];  // LDS byte offsets of the two decoded chunks of each piece inside a K (or V) image
#pragma unroll
  for (int i = 0; i < NP; ++i)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int row = prow + 32 * i;
      soff[i][c] = row * ROWB + 16 * ((2 * c16 + c) ^ pp_swz(row));
    }

  // ---- the block walk.  stage() is called once per tile, in key order, before that tile's loads.
  const int32_t* btr = bt + (size_t)slot * maxb;
  const int tpb = blk / BN;               // tiles per block
  const int nb = (Sk + blk - 1) / blk;    // blocks of the slot this segment reads
  int t_in = tpb, jb = -1;                // tile inside the block, block index: the first stage() enters block 0
  int bid_nx = btr[0];                    // id of block jb + 1
  const uint8_t* kblk = KC;
  const uint8_t* vblk = VC;
  const float* ksblk = KS_;
  const float* vsblk = VS_;
  int rlast = 0, trow = 0;
  auto stage = [&]() {
    if (t_in == tpb) {
      t_in = 0;
      ++jb;
      const int b = min(max(pp8_uniform(bid_nx), 0), blocks - 1);  // wave-uniform, inside the pool
      const size_t roff = ((size_t)b * Hkv + hk) * (size_t)blk;   // first row of the block, in rows
      kblk = KC + roff * D;
      vblk = VC + roff * D;
      ksblk = KS_ + roff;
      vsblk = VS_ + roff;
      rlast = min(blk, Sk - jb * blk) - 1;  // the last row of the block that the segment may see
      bid_nx = btr[min(jb + 1, nb - 1)];
    }
    trow = t_in * BN;
    ++t_in;
  };
  // the staged tile's codes and scales, HBM -> registers
  uint4 kreg[NP], vreg[NP];
  float kscl[NP], vscl[NP];
  auto load_tile = [&]() {
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int row = min(trow + prow + 32 * i, rlast);  // dead rows are never loaded
      kreg[i] = *reinterpret_cast<const uint4*>(kblk + row * D + 16 * c16);
      kscl[i] = ksblk[row];
    }
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int row = min(trow + prow + 32 * i, rlast);
      vreg[i] = *reinterpret_cast<const uint4*>(vblk + row * D + 16 * c16);
      vscl[i] = vsblk[row];
    }
  };
  // registers -> bf16 -> ring slot buf: piece i of K (isv 0) or of V (isv 1)
  auto decode_piece = [&](int buf, int isv, int i) {
    char* img = smem + (buf * 2 + isv) * TILE;
    const uint4 c = isv ? vreg[i] : kreg[i];
    const float sc = isv ? vscl[i] : kscl[i];
    *reinterpret_cast<u16x8*>(img + soff[i][0]) = pp8_dec8(c.x, c.y, sc);
    *reinterpret_cast<u16x8*>(img + soff[i][1]) = pp8_dec8(c.z, c.w, sc);
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
  load_tile();
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    decode_piece(0, 0, i);
    decode_piece(0, 1, i);
  }
  // Q is in its registers before the loop: were its loads still counted inside, every k-step of every tile
  // would wait on vmcnt and drag the next tile's loads with it
#pragma unroll
  for (int s = 0; s < KS; ++s) pin(qf[s]);
  __syncthreads();
  const int wq_hi = q0 + 32 * w + 31;

  auto tile = [&](auto cur_c, int kt) {
    constexpr int CUR = decltype(cur_c)::value;
    constexpr int NXT = CUR ^ 1;
    constexpr int KOF = CUR * 2 * TILE;
    const bool more = kt + 1 < ntiles;
    const bool active = kt * BN <= wq_hi + p0;
    if (more) {
      stage();
      load_tile();  // tile kt + 1: in flight under this tile's QK^T
    }
    if (more && !active) {
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        decode_piece(NXT, 0, i);
        decode_piece(NXT, 1, i);
      }
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
        sacc[0] = pp8_mfma32(x[0], qf[st], sacc[0]);
        sacc[1] = pp8_mfma32(x[1], qf[st], sacc[1]);
        // the next tile's K pieces, in the second half of the k-steps (their loads came first)
        if (more && st >= KS / 2 && (st - KS / 2) % (KS / 2 / NP) == 0) decode_piece(NXT, 0, (st - KS / 2) / (KS / 2 / NP));
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
            o[db] = pp8_mfma32(a, pb, o[db]);
          }
          // the next tile's V pieces, one after each of the first NP PV groups
          if (more && 2 * nn + s2 < NP) decode_piece(NXT, 1, 2 * nn + s2);
        }
    }
    __syncthreads();  // every wave's stores of tile kt + 1 are in LDS; slot CUR is free again
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

extern "C" int mx_prefill_attn_paged_kv8(const mx::PpKv8Launch& L, float scale, hipStream_t stream) {
  if (L.nseg <= 0) return 0;
  if (!pp8_takes(L)) return -1;
  const float sl = scale * 1.4426950408889634f;
  prefill_paged_kv8_kernel<<<(unsigned)(L.nwork * L.Hq), 256, 0, stream>>>(
      (const uint16_t*)L.q, (const uint8_t*)L.k_codes.p, (const float*)L.k_scale.p, (const uint8_t*)L.v_codes.p,
      (const float*)L.v_scale.p, (uint16_t*)L.o, L.bt, L.segs, L.work, (int)L.Hq, (int)L.k_codes.dim[1],
      (int)L.k_codes.dim[0], (int)L.k_codes.dim[2], (int)L.maxb, sl, (int)L.ldo);
  return (int)hipGetLastError();
}
