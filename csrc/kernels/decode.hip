// Inference-side kernels for gfx950:
//   * rope_append : decode-step q/k RoPE at per-sequence positions + KV-cache append
//   * decode_attn : single-token GQA attention over a per-slot KV cache,
//                   split over the sequence (flash-decoding), memory-bound:
//                   each workgroup streams 256 keys of one (seq, kv-head) once
//                   and serves all q-heads of that group (GQA reuse);
//   * decode_combine : merges the per-split (m, l, o) partials;
//   * kv8_quant_rows / rope_append_kv8 / decode_attn_kv8 : the same append and attention
//                   over an fp8 (e4m3) cache with one power-of-two scale per row;
//   * verify_attn : decode_attn for up to n consecutive query rows per sequence (speculative
//                   decoding), both cache formats: the K/V are streamed once for all the rows;
//   * sample : greedy argmax or exact temperature sampling via Gumbel-max with
//              a counter-based hash RNG (one pass, no softmax materialised).
// KV cache layout per layer: [slots, Hkv, max_seq, D] bf16 (contiguous per slot
// and head: one 256-B row per token for D = 128), or PAGED: a pool of blocks
// [blocks, Hkv, block, D] addressed through a per-slot block table (common.h
// kv_row; the block size is a multiple of the 256-key decode split, so every
// split reads one contiguous block).
#include "bindings.h"
#include "common.h"

namespace mx {

// Item i of a rope_append launch over qkv [B, NH * D]: D / 16 items per (row b, head), each with
// the value chunks c and c + D / 2 (8 values each) of a rotation pair
template <int D>
struct RopeItem {
  static constexpr int HALF = D / 2, CPH = HALF / 8;
  int b, head, c, p, slot;
  u16x8 x1, x2;
  __device__ __forceinline__ RopeItem(int64_t i, const uint16_t* __restrict__ qkv, const int32_t* __restrict__ pos,
                                      const int32_t* __restrict__ slots, int NH) {
    c = (int)(i % CPH) * 8;
    head = (int)((i / CPH) % NH);
    b = (int)(i / ((int64_t)CPH * NH));
    p = pos[b];
    slot = slots ? slots[b] : b;
    const uint16_t* src = qkv + (int64_t)b * NH * D + (int64_t)head * D;
    x1 = *reinterpret_cast<const u16x8*>(src + c);
    x2 = *reinterpret_cast<const u16x8*>(src + HALF + c);
  }
  // (x1, x2) rotated by the angles of position p
  __device__ __forceinline__ void rotate(const float* __restrict__ cosb, const float* __restrict__ sinb, u16x8& y1,
                                         u16x8& y2) const {
    const float* cp = cosb + (int64_t)p * HALF + c;
    const float* sp = sinb + (int64_t)p * HALF + c;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float a = bf2f(x1[j]), bb = bf2f(x2[j]);
      y1[j] = f2bf(a * cp[j] - bb * sp[j]);
      y2[j] = f2bf(bb * cp[j] + a * sp[j]);
    }
  }
};

// qkv [B, (Hq+2Hkv)*D] -> q [B, Hq, D] (rotated), K/V cache rows at pos[b]
template <int D>
__global__ void __launch_bounds__(256) rope_append_kernel(const uint16_t* __restrict__ qkv,
                                                          const float* __restrict__ cosb,
                                                          const float* __restrict__ sinb,
                                                          const int32_t* __restrict__ pos,
                                                          const int32_t* __restrict__ slots,
                                                          uint16_t* __restrict__ q, uint16_t* __restrict__ kc,
                                                          uint16_t* __restrict__ vc, int B, int Hq, int Hkv,
                                                          int max_seq, const int32_t* __restrict__ bt, int maxb) {
  constexpr int HALF = D / 2, CPH = HALF / 8;
  const int NH = Hq + 2 * Hkv;
  const int64_t n = (int64_t)B * NH * CPH;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const RopeItem<D> it(i, qkv, pos, slots, NH);
    const int head = it.head, c = it.c;
    uint16_t* dst;
    if (head >= Hq + Hkv) {
      dst = vc + kv_row(bt, maxb, max_seq, it.slot, Hkv, head - Hq - Hkv, it.p) * D;
      *reinterpret_cast<u16x8*>(dst + c) = it.x1;
      *reinterpret_cast<u16x8*>(dst + HALF + c) = it.x2;
      continue;
    }
    dst = head < Hq ? q + ((int64_t)it.b * Hq + head) * D
                    : kc + kv_row(bt, maxb, max_seq, it.slot, Hkv, head - Hq, it.p) * D;
    u16x8 y1, y2;
    it.rotate(cosb, sinb, y1, y2);
    *reinterpret_cast<u16x8*>(dst + c) = y1;
    *reinterpret_cast<u16x8*>(dst + HALF + c) = y2;
  }
}

constexpr int kSplit = 256;  // keys per workgroup
constexpr int kMaxRep = 16;  // q-heads per kv-head supported

// stores / loads of the split partials that another workgroup of the SAME launch merges:
// write-through (sc1, relaxed agent-scope atomic store), so no release fence (an L2
// write-back per workgroup) is needed, and loads that bypass this CU's L1 (guide
// §6 Guideline 16, the sc1 hand-off form)
// st: 0 = plain store, 1 = agent-scope relaxed atomic store (sc1 write-through),
// 2 = system-scope relaxed atomic store; ld: 0 = plain load, 1 = agent, 2 = system
__device__ __forceinline__ void st_part(float* p, float v, int st) {
  if (st == 1) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else if (st == 2) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  else *p = v;
}
__device__ __forceinline__ float ld_part(const float* p, int ld) {
  float* q = const_cast<float*>(p);
  if (ld == 1) return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (ld == 2) return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  return *p;
}

// The work of one workgroup of a decode-attention grid (nsplit, Hkv, B): keys k_lo .. k_hi - 1 of
// cache slot `slot`, kv-head hk, for the rep q-heads of its GQA group.  pml: the group's first
// head's (m, l) of this split; head h at + h * nsplit * 2.
struct DecodeSplit {
  int split, hk, b, rep, slot, k_lo, k_hi;
  float* pml;
  // verify_attn only (verify_split_begin): n rows per sequence in the launch, nq of them in use,
  // row j sees keys 0 .. len0 + j - 1
  int n, nq, len0;
};
// false for an empty split (workgroup-uniform), whose neutral partial is stored here (mode st)
__device__ __forceinline__ bool decode_split_begin(DecodeSplit& s, const int32_t* __restrict__ lens, int len_off,
                                                   const int32_t* __restrict__ slots, float* __restrict__ part_ml,
                                                   int Hq, int Hkv, int nsplit, int st) {
  s.split = blockIdx.x, s.hk = blockIdx.y, s.b = blockIdx.z;
  s.rep = Hq / Hkv;
  const int len = lens[s.b] + len_off;
  s.slot = slots ? slots[s.b] : s.b;
  s.k_lo = s.split * kSplit;
  s.k_hi = min(len, s.k_lo + kSplit);
  s.pml = part_ml + (((int64_t)s.b * Hq + s.hk * s.rep) * nsplit + s.split) * 2;
  if (s.k_lo < s.k_hi) return true;
  const int tid = threadIdx.x;
  if (tid < s.rep) {
    st_part(&s.pml[(int64_t)tid * nsplit * 2], -INFINITY, st);
    st_part(&s.pml[(int64_t)tid * nsplit * 2 + 1], 0.f, st);
  }
  return false;
}

// grid (nsplit, Hkv, B); block 256 = one key per thread for the score phase.
template <int D>
__global__ void __launch_bounds__(256) decode_attn_kernel(const uint16_t* __restrict__ q,
                                                          const uint16_t* __restrict__ kc,
                                                          const uint16_t* __restrict__ vc,
                                                          const int32_t* __restrict__ lens, int len_off,
                                                          const int32_t* __restrict__ slots,
                                                          float* __restrict__ part_ml, float* __restrict__ part_o,
                                                          int Hq, int Hkv, int max_seq, int nsplit, float sl,
                                                          const int32_t* __restrict__ bt, int maxb) {
  __shared__ float qs[kMaxRep][D];
  __shared__ float ps[kMaxRep][kSplit];
  __shared__ float red[kMaxRep][4];
  __shared__ __attribute__((aligned(16))) uint16_t vs[kSplit * D];
  DecodeSplit ds;
  if (!decode_split_begin(ds, lens, len_off, slots, part_ml, Hq, Hkv, nsplit, 0)) return;
  const int split = ds.split, hk = ds.hk, b = ds.b, rep = ds.rep, slot = ds.slot, k_lo = ds.k_lo, k_hi = ds.k_hi;
  float* pml = ds.pml;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  for (int i = tid; i < rep * D; i += 256) {
    const int h = i / D, d = i % D;
    qs[h][d] = bf2f(q[((int64_t)b * Hq + hk * rep + h) * D + d]);
  }
  // base such that base + key * D addresses every key of this split (a paged split lies in
  // one block: the block size is a multiple of kSplit)
  const int64_t kvb = (kv_row(bt, maxb, max_seq, slot, Hkv, hk, k_lo) - k_lo) * D;
  const uint16_t* kbase = kc + kvb;
  const uint16_t* vbase = vc + kvb;
  // stage V rows of this split into LDS (coalesced 16-B chunks)
  constexpr int CH = D / 8;
  for (int c = tid; c < kSplit * CH; c += 256) {
    const int row = c / CH, ch = c % CH, key = k_lo + row;
    u16x8 v = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (key < k_hi) v = *reinterpret_cast<const u16x8*>(vbase + (int64_t)key * D + ch * 8);
    *reinterpret_cast<u16x8*>(vs + row * D + ch * 8) = v;
  }
  __syncthreads();
  const int key = k_lo + tid;
  float s[kMaxRep];
#pragma unroll
  for (int h = 0; h < kMaxRep; ++h) s[h] = -INFINITY;
  if (key < k_hi) {
#pragma unroll
    for (int h = 0; h < kMaxRep; ++h) s[h] = 0.f;
    const uint16_t* kr = kbase + (int64_t)key * D;
#pragma unroll 4
    for (int c = 0; c < D; c += 8) {
      const u16x8 kv = *reinterpret_cast<const u16x8*>(kr + c);
      float kf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) kf[j] = bf2f(kv[j]);
#pragma unroll
      for (int h = 0; h < kMaxRep; ++h) {
        if (h < rep) {
#pragma unroll
          for (int j = 0; j < 8; ++j) s[h] += qs[h][c + j] * kf[j];
        }
      }
    }
#pragma unroll
    for (int h = 0; h < kMaxRep; ++h) s[h] *= sl;
  }
  // per-head max over the split
#pragma unroll
  for (int h = 0; h < kMaxRep; ++h) {
    if (h < rep) {
      const float m = wave_max(s[h]);
      if (lane == 0) red[h][wid] = m;
    }
  }
  __syncthreads();
  float mh[kMaxRep];
#pragma unroll
  for (int h = 0; h < kMaxRep; ++h)
    mh[h] = h < rep ? fmaxf(fmaxf(red[h][0], red[h][1]), fmaxf(red[h][2], red[h][3])) : 0.f;
  __syncthreads();
#pragma unroll
  for (int h = 0; h < kMaxRep; ++h) {
    if (h < rep) {
      const float p = key < k_hi ? __builtin_amdgcn_exp2f(s[h] - mh[h]) : 0.f;
      ps[h][tid] = p;
      const float l = wave_sum(p);
      if (lane == 0) red[h][wid] = l;
    }
  }
  __syncthreads();
  if (tid < rep) {
    pml[(int64_t)tid * nsplit * 2] = mh[tid];
    pml[(int64_t)tid * nsplit * 2 + 1] = red[tid][0] + red[tid][1] + red[tid][2] + red[tid][3];
  }
  // o[h][d] = sum_key p[h][key] v[key][d]: thread -> (h, d pair)
  const int nkeys = k_hi - k_lo;
  for (int o = tid; o < rep * (D / 2); o += 256) {
    const int h = o / (D / 2), d = (o % (D / 2)) * 2;
    float a0 = 0.f, a1 = 0.f;
    for (int kk = 0; kk < nkeys; ++kk) {
      const float p = ps[h][kk];
      const uint32_t pr = *reinterpret_cast<const uint32_t*>(vs + kk * D + d);
      a0 += p * bf2f((uint16_t)(pr & 0xffff));
      a1 += p * bf2f((uint16_t)(pr >> 16));
    }
    float* po = part_o + ((((int64_t)b * Hq + hk * rep + h) * nsplit + split) * D) + d;
    po[0] = a0;
    po[1] = a1;
  }
}

// ---------------------------------------------------------------------------
// MFMA decode attention, D = 128 (every Llama-3.x model).  Memory-bound: the
// whole point is to stream each (seq, kv-head)'s cached K/V rows once at HBM
// rate, so
//   * a workgroup = 4 waves = 256 keys of one (seq, kv-head); each wave owns 64
//     keys and keeps its own online-softmax state (no barrier in the key loop);
//   * scores for ALL q-heads of the GQA group at once with
//     v_mfma_f32_16x16x32_bf16: S^T[key][head] = K . Q^T, K rows loaded straight
//     from HBM into the A fragments (16 B per lane), Q^T (heads padded to 16)
//     as the B fragment;
//   * the S^T accumulator (head on the lane, keys in registers) converted to
//     bf16 IS the B operand of O^T[d][head] += V^T . P (keys permuted inside
//     each 32-key k-step to match the accumulator's row order);
//   * V^T fragments come from a row-major V image in LDS through
//     ds_read_b64_tr_b16; the image is filled by LDS-DMA (global_load_lds,
//     source-swizzled so the transposed reads are conflict-free);
//   * the four waves' partials are merged through LDS (each wave reuses its own
//     V region) into one (m, l, o) partial per split, the format of
//     decode_combine_kernel.
// 64 KiB LDS and < 128 VGPRs: two workgroups (8 waves) per CU, 256 KiB of K/V
// in flight per CU.
// decode_split_body is a template over the cache format: how K and V reach the
// fragments and the image above is KvBf16's; KvFp8 (kv8 section) decodes e4m3
// codes on the way.  Everything from the softmax on exists once.
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

__device__ __forceinline__ f32x4 mfma16(const u16x8& a, const u16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b),
                                                 c, 0, 0, 0);
}

__device__ __forceinline__ u16x4 tr_read16(const char* p) {
  s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p));
  return __builtin_bit_cast(u16x4, v);
}

// 16-B chunk swizzle of a 256-B row (conflict-free row and transposed reads)
__device__ __forceinline__ int dswz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }

// What decode_split_body needs from a cache format (this one and KvFp8 below).  rb + key is the
// cache row of every key of the split (kv_row: a split lies in one block); lane = (c, g) = (lane &
// 15, lane >> 4); the wave's keys are wk0 .. wk0 + 63 and its 16-KiB LDS region is vs.  Keys at or
// past k_hi are never loaded: the index is clamped to k_hi - 1.
//   * load_v: issues the loads of the wave's V rows; finish_v: the swizzled bf16 V image (rows of
//     256 B, 16-B chunks permuted by dswz) is complete in vs.  Rows past k_hi duplicate a valid
//     row (finite; their probabilities are exactly 0);
//   * load_k: issues the loads of the K operands; k_frag(j, s): the A fragment of block j, k-step s,
//     K[wk0 + 16 j + c][q_col(s, g) .. +7];
//   * q_col(s, g): the first of the 8 dimensions that k-step s covers for lane group g (the MFMA
//     summation order of the format);
//   * score(x, j, i): x times the format's factor for key wk0 + 16 j + 4 g + i;
//   * kQFirst: Q is loaded before K (the order of the loads as each format was tuned);
//   * kMergeFma: the wave merge accumulates O with fused multiply-adds (true) or rounds each
//     product first (false): the arithmetic each format's decode kernel has always had, now
//     written out so that every instantiation of the body over the format has it.
//
// bf16 cache: K rows go straight from HBM into the A fragments (16 B per lane), V rows to LDS by
// LDS-DMA (16 x 1-KiB lane-linear pieces; swizzle by permuting each lane's SOURCE chunk).
struct KvBf16 {
  static constexpr bool kQFirst = true, kMergeFma = true;
  const uint16_t* kc;
  const uint16_t* vc;
  u16x8 kf[4][4];
  __device__ __forceinline__ void load_v(int64_t rb, int wk0, int k_hi, int lane, char* vs) {
    const uint16_t* vbase = vc + rb * 128;
#pragma unroll
    for (int seg = 0; seg < 16; ++seg) {
      const int row = seg * 4 + (lane >> 4), slt = lane & 15;
      const int ch = slt ^ dswz(row);
      const int key = min(wk0 + row, k_hi - 1);
      __builtin_amdgcn_global_load_lds((gptr_t)(vbase + (int64_t)key * 128 + ch * 8), (lptr_t)(vs + seg * 1024), 16,
                                       0, 0);
    }
  }
  __device__ __forceinline__ void finish_v(int, char*) {
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): this wave's V DMA has landed (only it reads vs)
  }
  __device__ __forceinline__ void load_k(int64_t rb, int wk0, int k_hi, int c, int g) {
    const uint16_t* kbase = kc + rb * 128;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = min(wk0 + 16 * j + c, k_hi - 1);
#pragma unroll
      for (int s = 0; s < 4; ++s) kf[j][s] = *reinterpret_cast<const u16x8*>(kbase + (int64_t)key * 128 + q_col(s, g));
    }
  }
  __device__ __forceinline__ u16x8 k_frag(int j, int s) const { return kf[j][s]; }
  static __device__ __forceinline__ int q_col(int s, int g) { return 32 * s + 8 * g; }
  __device__ __forceinline__ float score(float x, int, int) const { return x; }
};

// one split of a decode-attention kernel over a cache of format KV: (m, l, o) partial of 256 keys
// for every column of the (sequence, KV head) (see the header comment above), stored in mode st.
// The 16 MFMA columns of a block are the q-heads of the GQA group (ROWS = false: decode, one query
// row per sequence, NB = 1), or (query row j, head h) pairs, column col = j * rep + h over NB blocks
// of 16 (ROWS = true: verify_attn).  A column has its own key limit (row j sees keys < len0 + j),
// its own Q row and its own partial, (m, l, o) of q row b * n + j; the blocks share the K fragments
// and the V image and have separate score and output accumulators.  Keys past a column's limit
// but inside the split are real rows: their scores are replaced by -inf, their P is exactly 0.
template <class KV, int NB = 1, bool ROWS = false>
__device__ __forceinline__ void decode_split_body(const uint16_t* __restrict__ q, KV& kv, float* __restrict__ part_o,
                                                  const DecodeSplit& ds, char* smem, float (*mls)[2][16 * NB], int Hq,
                                                  int Hkv, int nsplit, int max_seq, float sl,
                                                  const int32_t* __restrict__ bt, int maxb, int st) {
  // Every instantiation rounds alike: nothing here is contracted by the compiler's choice (which
  // differs between instantiations -- a packed multiply in one, a fused multiply-add in the
  // next); where the kernels have always fused, the fma is written out (the wave merge below).
#pragma clang fp contract(off)
  static_assert(ROWS || NB == 1, "decode: one block of columns");
  constexpr int D = 128, ROWB = 256, WKEYS = 64, WTILE = WKEYS * ROWB, NC = 16 * NB;
  const int b = ds.b, hk = ds.hk, rep = ds.rep, split = ds.split, k_lo = ds.k_lo, k_hi = ds.k_hi;
  float* pml = ds.pml;
  const int ncols = ROWS ? ds.n * rep : rep;
  // (q row, head) index of column col: where its Q row, its partial and its output live
  auto col_bh = [&](int col) -> int64_t {
    if constexpr (ROWS) return ((int64_t)b * ds.n + col / rep) * Hq + hk * rep + col % rep;
    else return (int64_t)b * Hq + hk * rep + col;
  };
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int64_t rb = kv_row(bt, maxb, max_seq, ds.slot, Hkv, hk, k_lo) - k_lo;  // one block per split
  const int wk0 = k_lo + WKEYS * w;
  char* vs = smem + w * WTILE;

  kv.load_v(rb, wk0, k_hi, lane, vs);
  if constexpr (!KV::kQFirst) kv.load_k(rb, wk0, k_hi, c, g);
  // Q^T fragments (B operand): lane (c, g), k-step s holds Q[head c][q_col(s, g) .. +7]
  // klim: the keys that this lane's column sees end here (a column past ncols or of a row that is
  // not in use sees none)
  u16x8 qf[NB][4];
  int klim[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int col = 16 * nb + c;
    bool on = col < ncols;
    klim[nb] = k_hi;
    if constexpr (ROWS) {
      const int j = col / rep;
      on = on && j < ds.nq;
      klim[nb] = on ? min(k_hi, ds.len0 + j) : 0;
    }
    const uint16_t* qrow = q + col_bh(min(col, ncols - 1)) * D;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      qf[nb][s] = *reinterpret_cast<const u16x8*>(qrow + KV::q_col(s, g));
      if (!on) qf[nb][s] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }
  if constexpr (KV::kQFirst) kv.load_k(rb, wk0, k_hi, c, g);
  f32x4 sacc[NB][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) sacc[nb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const u16x8 kf = kv.k_frag(j, s);
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) sacc[nb][j] = mfma16(kf, qf[nb][s], sacc[nb][j]);
    }
  }
  // Nothing is scheduled across this point, so every load of the split is in flight before the
  // softmax.  Loads to here and softmax are one basic block, and without the barrier the scheduler
  // sinks two of KvFp8's V loads (and their scales) to just before finish_v, where nothing hides
  // their latency.
  __builtin_amdgcn_sched_barrier(0);
  // softmax over this wave's 64 keys, per column (= lane column c of each block); lane (c, g)
  // holds keys wk0 + 16 j + 4 g + i
  float mx[NB], ls[NB];
  u16x8 pb[NB][2];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = wk0 + 16 * j + 4 * g + i;
        const float x = key < klim[nb] ? kv.score(sacc[nb][j][i], j, i) * sl : -INFINITY;
        sacc[nb][j][i] = x;
        m = fmaxf(m, x);
      }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const float mref = m == -INFINITY ? 0.f : m;  // wave with no valid key: all p = 0
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = __builtin_amdgcn_exp2f(sacc[nb][j][i] - mref);
        l += p;
        pb[nb][j >> 1][4 * (j & 1) + i] = f2bf(p);
      }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    mx[nb] = m, ls[nb] = l;
  }

  // O^T[d][column] += V^T . P; k-step t covers keys 32 t + {16 h + 4 g + i}.  Only this wave
  // reads its image, and a wave's LDS operations complete in order.
  f32x4 oacc[NB][8];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int db = 0; db < 8; ++db) oacc[nb][db] = f32x4{0.f, 0.f, 0.f, 0.f};
  kv.finish_v(lane, vs);
  const int qq = c >> 2, pp = c & 3;
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const int r0 = 32 * t + 4 * g + qq, r1 = r0 + 16;
#pragma unroll
    for (int db = 0; db < 8; ++db) {
      const int ch = 2 * db + (pp >> 1);
      const u16x4 va = tr_read16(vs + r0 * ROWB + 16 * (ch ^ dswz(r0)) + 8 * (pp & 1));
      const u16x4 vb = tr_read16(vs + r1 * ROWB + 16 * (ch ^ dswz(r1)) + 8 * (pp & 1));
      const u16x8 a = u16x8{va[0], va[1], va[2], va[3], vb[0], vb[1], vb[2], vb[3]};
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) oacc[nb][db] = mfma16(a, pb[nb][t], oacc[nb][db]);
    }
  }
  // merge the four waves: each wave parks (m, l, O^T) in its own V region
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): this wave's transposed reads retired
  float* so = reinterpret_cast<float*>(vs);  // [d][NC columns]: NB = 2 fills the wave's 16 KiB
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
    for (int db = 0; db < 8; ++db)
#pragma unroll
      for (int i = 0; i < 4; ++i) so[(16 * db + 4 * g + i) * NC + 16 * nb + c] = oacc[nb][db][i];
    if (g == 0) {
      mls[w][0][16 * nb + c] = mx[nb];
      mls[w][1][16 * nb + c] = ls[nb];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < ncols * D; idx += 256) {
    const int h = idx / D, d = idx % D;  // h: the column
    float M = -INFINITY;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) M = fmaxf(M, mls[ww][0][h]);
    float L = 0.f, acc = 0.f;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) {
      const float mw = mls[ww][0][h];
      const float f = mw == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mw - M);
      const float ow = reinterpret_cast<const float*>(smem + ww * WTILE)[d * NC + h];
      L = __builtin_fmaf(f, mls[ww][1][h], L);
      if constexpr (KV::kMergeFma) acc = __builtin_fmaf(f, ow, acc);
      else acc = acc + f * ow;
    }
    const int64_t bh = col_bh(h);
    st_part(&part_o[(bh * nsplit + split) * D + d], acc, st);
    if (d == 0) {
      // ROWS: pml is split `split` of (row 0, head 0); decode: of the group's first head
      float* ml = ROWS ? pml + bh * nsplit * 2 : pml + (int64_t)h * nsplit * 2;
      st_part(&ml[0], M, st);
      st_part(&ml[1], L, st);
    }
  }
}

// One output value from its nsplit partials, ml = (m, l) pairs and po = o values D floats apart,
// loaded in mode LD (ld_part): the maximum over the splits, then weights, L and acc in split order.
// The in-launch merger and decode_combine_kernel both use it, so they agree bit for bit.
template <int LD>
__device__ __forceinline__ float merge_splits(const float* ml, const float* po, int nsplit, int D) {
  float M = -INFINITY;
  for (int s = 0; s < nsplit; ++s) M = fmaxf(M, ld_part(ml + 2 * s, LD));
  float L = 0.f, acc = 0.f;
  for (int s = 0; s < nsplit; ++s) {
    const float m = ld_part(ml + 2 * s, LD);
    if (m == -INFINITY) continue;
    const float wgt = __builtin_amdgcn_exp2f(m - M);
    L += wgt * ld_part(ml + 2 * s + 1, LD);
    acc += wgt * ld_part(po + (int64_t)s * D, LD);
  }
  return L > 0.f ? acc / L : 0.f;
}

// proto (fused split merge, cnt != nullptr; 0 = partials only / combine kernel):
//   1 = partials stored with agent-scope (sc1, write-through) atomic stores, read back with
//       agent-scope atomic loads, no fences;
//   2 = the same at system scope;
//   3 = agent-scope stores, an agent-scope acquire fence in the merger, plain loads;
//   4 = plain stores, one agent-scope release fence per workgroup (lane 0, after every wave's
//       vmcnt drain), acquire fence in the merger, plain loads (guide §5 in-launch split-K recipe).
__global__ void __launch_bounds__(256, 2) decode_attn_mfma_kernel(const uint16_t* __restrict__ q,
                                                                  const uint16_t* __restrict__ kc,
                                                                  const uint16_t* __restrict__ vc,
                                                                  const int32_t* __restrict__ lens, int len_off,
                                                                  const int32_t* __restrict__ slots,
                                                                  float* __restrict__ part_ml,
                                                                  float* __restrict__ part_o, int Hq, int Hkv,
                                                                  int max_seq, int nsplit, float sl,
                                                                  const int32_t* __restrict__ bt, int maxb,
                                                                  uint16_t* __restrict__ out,
                                                                  unsigned int* __restrict__ cnt, int proto) {
  constexpr int D = 128, WTILE = 64 * 256;  // 16 KiB per wave
  __shared__ __attribute__((aligned(16))) char smem[4 * WTILE];
  __shared__ float mls[4][2][16];
  __shared__ int s_last;
  const int tid = threadIdx.x;
  const bool fused = cnt != nullptr;
  const int st = !fused ? 0 : proto == 2 ? 2 : proto == 4 ? 0 : 1;  // store mode of the partials
  DecodeSplit ds;
  if (decode_split_begin(ds, lens, len_off, slots, part_ml, Hq, Hkv, nsplit, st)) {
    KvBf16 kv{kc, vc};
    decode_split_body(q, kv, part_o, ds, smem, mls, Hq, Hkv, nsplit, max_seq, sl, bt, maxb, st);
  }
  if (!fused) return;
  const int hk = ds.hk, b = ds.b, rep = ds.rep;
  // In-launch combine: the last of the nsplit workgroups of this (seq, kv-head) to arrive
  // merges the partials and resets the counter (zero again for the next call).
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave: its partial stores done
  __syncthreads();
  if (tid == 0) {
    unsigned int* c = cnt + (int64_t)b * Hkv + hk;
    if (proto == 4) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const unsigned prev = proto == 2 ? __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)
                                     : __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int last = prev == (unsigned)(nsplit - 1);
    if (last) {
      __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (proto >= 3) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
    }
    s_last = last;
  }
  __syncthreads();
  if (!s_last) return;
  for (int idx = tid; idx < rep * D; idx += 256) {
    const int h = idx / D, d = idx % D;
    const int64_t bh = (int64_t)b * Hq + hk * rep + h;
    const float* ml = part_ml + bh * nsplit * 2;
    const float* po = part_o + bh * nsplit * D + d;
    const float o = proto == 1 ? merge_splits<1>(ml, po, nsplit, D)
                  : proto == 2 ? merge_splits<2>(ml, po, nsplit, D)
                               : merge_splits<0>(ml, po, nsplit, D);
    out[bh * D + d] = f2bf(o);
  }
}

// merge splits: out[b, h, :] = sum_s exp2(m_s - M) o_s / sum_s exp2(m_s - M) l_s
template <int D>
__global__ void __launch_bounds__(D) decode_combine_kernel(const float* __restrict__ part_ml,
                                                           const float* __restrict__ part_o,
                                                           uint16_t* __restrict__ out, int nsplit) {
  const int64_t bh = blockIdx.x;
  const float* ml = part_ml + bh * nsplit * 2;
  const int d = threadIdx.x;
  if (nsplit <= 8) {
    // every partial load issued at once (one memory round trip instead of two: the outputs'
    // loads do not wait for the maxima); same arithmetic order as merge_splits
    float mv[8], lv[8], ov[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const bool on = s < nsplit;
      mv[s] = on ? ml[2 * s] : -INFINITY;
      lv[s] = on ? ml[2 * s + 1] : 0.f;
      ov[s] = on ? part_o[(bh * nsplit + s) * D + d] : 0.f;
    }
    float M = -INFINITY;
#pragma unroll
    for (int s = 0; s < 8; ++s) M = fmaxf(M, mv[s]);
    float L = 0.f, acc = 0.f;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (mv[s] == -INFINITY) continue;
      const float wgt = __builtin_amdgcn_exp2f(mv[s] - M);
      L += wgt * lv[s];
      acc += wgt * ov[s];
    }
    out[bh * D + d] = f2bf(L > 0.f ? acc / L : 0.f);
    return;
  }
  out[bh * D + d] = f2bf(merge_splits<0>(ml, part_o + bh * nsplit * D + d, nsplit, D));
}

// ---------------------------------------------------------------------------
// kv8: fp8 (OCP e4m3) KV cache, head_dim 128 (format: mxllm/serve/quant.py kv8_quantize).
// A row = the 128 values of one (token, kv-head): 128 e4m3 codes and one f32 scale 2^e, the
// smallest power of two with amax / 2^e <= 448.  Code pools [rows, Hkv, SEQ, 128] u8 and scale
// pools [rows, Hkv, SEQ] f32 are both addressed by kv_row (x 128 and x 1).  x * 2^-e is exact, the
// hardware pack conversion rounds to nearest even and keeps zero and subnormals; code * 2^e is a
// bf16 value, so decoding is exact and the dequantised cache is a bf16 cache.
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int kKv8MinExp = -100;

// e of a row's scale 2^e from the largest bf16 magnitude of the row (its bits without the sign):
// amax = m 2^E, 1 <= m < 2: E - 8 if m <= 1.75, else E - 7
__device__ __forceinline__ int kv8_exp(uint32_t amax_bits) {
  if (amax_bits == 0) return 0;
  return max((int)(amax_bits >> 7) - 135 + ((amax_bits & 0x7Fu) > 0x60u ? 1 : 0), kKv8MinExp);
}
__device__ __forceinline__ float kv8_pow2(int e) { return __uint_as_float((uint32_t)(e + 127) << 23); }
__device__ __forceinline__ uint32_t kv8_amax8(const u16x8& v) {
  uint32_t a = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) a = max(a, (uint32_t)v[j] & 0x7FFFu);
  return a;
}
// 8 bf16 values times inv (a power of two) -> 8 e4m3 codes
__device__ __forceinline__ uint2 kv8_pack8(const u16x8& v, float inv) {
  int lo = 0, hi = 0;
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(v[0]) * inv, bf2f(v[1]) * inv, lo, false);
  lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(v[2]) * inv, bf2f(v[3]) * inv, lo, true);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(v[4]) * inv, bf2f(v[5]) * inv, hi, false);
  hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf2f(v[6]) * inv, bf2f(v[7]) * inv, hi, true);
  return make_uint2((uint32_t)lo, (uint32_t)hi);
}
// 8 e4m3 codes times sc (a power of two) -> 8 bf16: the hardware conversion is exact for every
// code (subnormals included) and the product has 4 significant bits, so the bf16 is the upper
// half of the f32
__device__ __forceinline__ uint32_t kv8_hi2(float a, float b) {
  return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
}
__device__ __forceinline__ u16x8 kv8_dec8(uint32_t lo, uint32_t hi, float sc) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
  return __builtin_bit_cast(u16x8, u32x4{kv8_hi2(a[0] * sc, a[1] * sc), kv8_hi2(b[0] * sc, b[1] * sc),
                                         kv8_hi2(c[0] * sc, c[1] * sc), kv8_hi2(d[0] * sc, d[1] * sc)});
}
__device__ __forceinline__ u16x8 kv8_dec8(uint32_t lo, uint32_t hi) {
  const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, false), b = __builtin_amdgcn_cvt_pk_f32_fp8((int)lo, true);
  const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, false), d = __builtin_amdgcn_cvt_pk_f32_fp8((int)hi, true);
  return __builtin_bit_cast(u16x8, u32x4{kv8_hi2(a[0], a[1]), kv8_hi2(b[0], b[1]), kv8_hi2(c[0], c[1]),
                                         kv8_hi2(d[0], d[1])});
}

// X [R, 128] bf16 rows (stride ldx) -> codes [R, 128], scales [R]: 16 lanes per row (8 values
// each), four rows per wave, the row's amax by shuffles inside the lane group
__global__ void __launch_bounds__(256) kv8_quant_rows_kernel(const uint16_t* __restrict__ X, int64_t ldx,
                                                             uint8_t* __restrict__ Q, float* __restrict__ S,
                                                             int64_t R) {
  const int64_t row = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int cc = threadIdx.x & 15;
  if (row >= R) return;  // whole 16-lane groups leave
  const u16x8 v = *reinterpret_cast<const u16x8*>(X + row * ldx + cc * 8);
  uint32_t am = kv8_amax8(v);
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) am = max(am, (uint32_t)__shfl_xor((int)am, o, 64));
  const int e = kv8_exp(am);
  *reinterpret_cast<uint2*>(Q + row * 128 + cc * 8) = kv8_pack8(v, kv8_pow2(-e));
  if (cc == 0) S[row] = kv8_pow2(e);
}

// rope_append_kernel<128> into a kv8 cache: the same items (8 lanes per (row, head), each with
// the value chunks c and c + 64 of a rotation pair) and the same arithmetic; the K row is rounded
// to bf16 as rope_append stores it and then quantised like a V row, the row's amax by shuffles
// over the 8 lanes.  q is rope_append's q.
__global__ void __launch_bounds__(256) rope_append_kv8_kernel(
    const uint16_t* __restrict__ qkv, const float* __restrict__ cosb, const float* __restrict__ sinb,
    const int32_t* __restrict__ pos, const int32_t* __restrict__ slots, uint16_t* __restrict__ q,
    uint8_t* __restrict__ kq, float* __restrict__ ks, uint8_t* __restrict__ vq, float* __restrict__ vs, int B, int Hq,
    int Hkv, int max_seq, const int32_t* __restrict__ bt, int maxb) {
  constexpr int D = 128, HALF = D / 2, CPH = HALF / 8;
  const int NH = Hq + 2 * Hkv;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * NH * CPH) return;  // whole 8-lane groups leave
  const RopeItem<D> it(i, qkv, pos, slots, NH);
  const int head = it.head, c = it.c;
  u16x8 y1 = it.x1, y2 = it.x2;
  if (head < Hq + Hkv) it.rotate(cosb, sinb, y1, y2);
  if (head < Hq) {
    uint16_t* dst = q + ((int64_t)it.b * Hq + head) * D;
    *reinterpret_cast<u16x8*>(dst + c) = y1;
    *reinterpret_cast<u16x8*>(dst + HALF + c) = y2;
    return;
  }
  uint32_t am = max(kv8_amax8(y1), kv8_amax8(y2));
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) am = max(am, (uint32_t)__shfl_xor((int)am, o, 64));
  const int e = kv8_exp(am);
  const float inv = kv8_pow2(-e);
  const bool isv = head >= Hq + Hkv;
  const int64_t r = kv_row(bt, maxb, max_seq, it.slot, Hkv, head - Hq - (isv ? Hkv : 0), it.p);
  uint8_t* dst = (isv ? vq : kq) + r * D;
  *reinterpret_cast<uint2*>(dst + c) = kv8_pack8(y1, inv);
  *reinterpret_cast<uint2*>(dst + HALF + c) = kv8_pack8(y2, inv);
  if (c == 0) (isv ? vs : ks)[r] = kv8_pow2(e);
}

// kv8 cache for decode_split_body (the interface: KvBf16).  What differs from the bf16 cache:
//   * K codes go from HBM into registers, 16 per lane and load: lane (c, g) holds
//     K[key][64 sp + 16 g .. +15]; k-step s = 2 sp + h takes its bytes 8 h .. 8 h + 7, decoded to
//     bf16 in registers, and the Q^T fragment of that k-step holds the same 8 dimensions;
//   * the score of a key is multiplied by the key's K scale (a power of two: exact) before the
//     softmax scale;
//   * V codes are loaded to registers (row 8 seg + lane / 8, 16 codes per lane), decoded,
//     multiplied by the row's V scale and written to the swizzled bf16 image that the
//     transposed reads expect.
// Keys at or past k_hi are never loaded, codes or scales: the index is clamped to k_hi - 1.
struct KvFp8 {
  static constexpr bool kQFirst = false, kMergeFma = false;
  const uint8_t* kq;
  const float* ksc;
  const uint8_t* vq;
  const float* vsc;
  u32x4 vreg[8], kreg[4][2];
  float vscl[8], kscl[4][4];
  __device__ __forceinline__ void load_v(int64_t rb, int wk0, int k_hi, int lane, char*) {
    const uint8_t* vbase = vq + rb * 128;
    const float* vsb = vsc + rb;
#pragma unroll
    for (int seg = 0; seg < 8; ++seg) {
      const int key = min(wk0 + seg * 8 + (lane >> 3), k_hi - 1);
      vreg[seg] = *reinterpret_cast<const u32x4*>(vbase + (int64_t)key * 128 + 16 * (lane & 7));
      vscl[seg] = vsb[key];
    }
  }
  __device__ __forceinline__ void finish_v(int lane, char* vs) {
#pragma unroll
    for (int seg = 0; seg < 8; ++seg) {
      const int row = seg * 8 + (lane >> 3), ch = 2 * (lane & 7);
      char* dst = vs + row * 256;
      *reinterpret_cast<u16x8*>(dst + 16 * (ch ^ dswz(row))) = kv8_dec8(vreg[seg][0], vreg[seg][1], vscl[seg]);
      *reinterpret_cast<u16x8*>(dst + 16 * ((ch + 1) ^ dswz(row))) = kv8_dec8(vreg[seg][2], vreg[seg][3], vscl[seg]);
    }
  }
  __device__ __forceinline__ void load_k(int64_t rb, int wk0, int k_hi, int c, int g) {
    const uint8_t* kbase = kq + rb * 128;
    const float* ksb = ksc + rb;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int key = min(wk0 + 16 * j + c, k_hi - 1);
#pragma unroll
      for (int sp = 0; sp < 2; ++sp)
        kreg[j][sp] = *reinterpret_cast<const u32x4*>(kbase + (int64_t)key * 128 + 64 * sp + 16 * g);
#pragma unroll
      for (int i = 0; i < 4; ++i) kscl[j][i] = ksb[min(wk0 + 16 * j + 4 * g + i, k_hi - 1)];
    }
  }
  __device__ __forceinline__ u16x8 k_frag(int j, int s) const {
    return kv8_dec8(kreg[j][s >> 1][2 * (s & 1)], kreg[j][s >> 1][2 * (s & 1) + 1]);
  }
  static __device__ __forceinline__ int q_col(int s, int g) { return 64 * (s >> 1) + 16 * g + 8 * (s & 1); }
  __device__ __forceinline__ float score(float x, int j, int i) const { return x * kscl[j][i]; }
};

// grid (nsplit, Hkv, B): the (m, l, o) partials of decode_attn_mfma_kernel over a kv8 cache,
// merged by decode_combine_kernel
__global__ void __launch_bounds__(256, 2) decode_attn_kv8_kernel(
    const uint16_t* __restrict__ q, const uint8_t* __restrict__ kq, const float* __restrict__ ksc,
    const uint8_t* __restrict__ vq, const float* __restrict__ vsc, const int32_t* __restrict__ lens, int len_off,
    const int32_t* __restrict__ slots, float* __restrict__ part_ml, float* __restrict__ part_o, int Hq, int Hkv,
    int max_seq, int nsplit, float sl, const int32_t* __restrict__ bt, int maxb) {
  constexpr int WTILE = 64 * 256;  // 16 KiB per wave
  __shared__ __attribute__((aligned(16))) char smem[4 * WTILE];
  __shared__ float mls[4][2][16];
  DecodeSplit ds;
  if (!decode_split_begin(ds, lens, len_off, slots, part_ml, Hq, Hkv, nsplit, 0)) return;
  KvFp8 kv{kq, ksc, vq, vsc};
  decode_split_body(q, kv, part_o, ds, smem, mls, Hq, Hkv, nsplit, max_seq, sl, bt, maxb, 0);
}

// ---------------------------------------------------------------------------
// verify_attn: decode attention for up to n consecutive query rows per sequence (speculative
// decoding: the rows are the last accepted token and the drafts that follow it).  Sequence b has
// nq[b] rows (0 .. n) at positions L_b .. L_b + nq[b] - 1 of its slot, L_b = lens[b]; their K/V are
// already appended; row j sees keys 0 .. L_b + j.  q [B * n, Hq, 128]: row b * n + j.
// The kernel is decode_split_body with ROWS = true: the K/V of a (sequence, KV head) are streamed
// once for all its rows (decode_attn over the same rows streams them once per row).  Grid
// (nsplit, Hkv, B) as decode; the split range comes from the longest row.  NB = 1: n * rep <= 16
// columns, NB = 2: <= 32.  Partials (m, l, o) of q row b * n + j in decode's format, merged by
// decode_combine_kernel; rows j >= nq[b] get partials that combine to zeros.  Columns are
// independent and masked probabilities are exactly 0, so row j equals decode_attn /
// decode_attn_kv8 of that row as a sequence of its own (same slot, lens = L_b + j, len_off 1, same
// nsplit) bit for bit.
// nq[b] is clamped into [0, n] and L_b into [0, capacity - nq[b]]: no key at or past the slot's
// capacity is ever addressed.
// Resources (hipcc -O3 --offload-arch=gfx950, the metadata of the generated assembly; LDS = 4 x 16 KiB
// V images + mls; decode_attn_mfma_kernel has 96 VGPRs, decode_attn_kv8_kernel 123):
//   KvBf16 NB = 1:  97 VGPRs, 0 B scratch, 66048 B LDS     KvBf16 NB = 2: 161 VGPRs, 0 B scratch, 66560 B LDS
//   KvFp8  NB = 1: 126 VGPRs, 0 B scratch, 66048 B LDS     KvFp8  NB = 2: 162 VGPRs, 0 B scratch, 66560 B LDS
// All within the 256 VGPRs of __launch_bounds__(256, 2): two workgroups per CU, as decode.
__device__ __forceinline__ bool verify_split_begin(DecodeSplit& s, const int32_t* __restrict__ lens,
                                                   const int32_t* __restrict__ nq,
                                                   const int32_t* __restrict__ slots, float* __restrict__ part_ml,
                                                   int Hq, int Hkv, int n, int nsplit, int cap) {
  s.split = blockIdx.x, s.hk = blockIdx.y, s.b = blockIdx.z;
  s.rep = Hq / Hkv;
  s.n = n;
  s.nq = min(max(nq[s.b], 0), min(n, cap));
  const int L = max(min(lens[s.b], cap - s.nq), 0);
  s.len0 = L + 1;
  s.slot = slots ? slots[s.b] : s.b;
  s.k_lo = s.split * kSplit;
  s.k_hi = min(s.nq ? L + s.nq : 0, s.k_lo + kSplit);  // a sequence without rows streams nothing
  s.pml = part_ml + (int64_t)s.split * 2;
  if (s.k_lo < s.k_hi) return true;
  const int tid = threadIdx.x;
  if (tid < n * s.rep) {
    float* ml = s.pml + (((int64_t)s.b * n + tid / s.rep) * Hq + s.hk * s.rep + tid % s.rep) * nsplit * 2;
    ml[0] = -INFINITY;
    ml[1] = 0.f;
  }
  return false;
}

// k / v: bf16 pools (KvBf16; ksc = vsc = nullptr) or e4m3 code pools with their scale pools (KvFp8)
template <class KV, int NB>
__global__ void __launch_bounds__(256, 2) verify_attn_kernel(
    const uint16_t* __restrict__ q, const void* __restrict__ k, const float* __restrict__ ksc,
    const void* __restrict__ v, const float* __restrict__ vsc, const int32_t* __restrict__ lens,
    const int32_t* __restrict__ nq, const int32_t* __restrict__ slots, float* __restrict__ part_ml,
    float* __restrict__ part_o, int Hq, int Hkv, int n, int max_seq, int nsplit, float sl,
    const int32_t* __restrict__ bt, int maxb) {
  constexpr int WTILE = 64 * 256;  // 16 KiB per wave
  __shared__ __attribute__((aligned(16))) char smem[4 * WTILE];
  __shared__ float mls[4][2][16 * NB];
  DecodeSplit ds;
  const int cap = bt ? maxb * max_seq : max_seq;
  if (!verify_split_begin(ds, lens, nq, slots, part_ml, Hq, Hkv, n, nsplit, cap)) return;
  if constexpr (std::is_same<KV, KvFp8>::value) {
    KvFp8 kv{(const uint8_t*)k, ksc, (const uint8_t*)v, vsc};
    decode_split_body<KvFp8, NB, true>(q, kv, part_o, ds, smem, mls, Hq, Hkv, nsplit, max_seq, sl, bt, maxb, 0);
  } else {
    KvBf16 kv{(const uint16_t*)k, (const uint16_t*)v};
    decode_split_body<KvBf16, NB, true>(q, kv, part_o, ds, smem, mls, Hq, Hkv, nsplit, max_seq, sl, bt, maxb, 0);
  }
}

// logits [B, V] (bf16 or f32); temperature <= 0 -> greedy.  out ids [B] int64.
//
// Split over the vocabulary: grid (nchunks, B), each workgroup reduces `chunk`
// logits of one row to (max, smallest index); a second one-wave-per-row kernel
// combines the partials in chunk order.  One workgroup per row left a batch-1
// decode step with ONE CU streaming 256 KB of logits: 176 us of a 4.1 ms 8B
// step; split over ~63 workgroups it is a few microseconds.  (A last-arriver
// merge in the same kernel needed an agent-scope release fence per workgroup:
// 94 us at batch 64.)  The result (and the Gumbel noise of each (seed, row,
// step, index)) is the same as a single-pass argmax.  The partials live in a
// per-call workspace (allocated by the caller on its stream), so concurrent
// samplers on different streams of one device never share them.
constexpr int kSampMaxRows = 1024;   // rows per launch (more rows: several launches)
constexpr int kSampMaxChunks = 64;   // partials per row (= one wave in the final pass)

__device__ __forceinline__ void samp_pick(float& best, int& bi, float ov, int oi) {
  if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
}

template <typename T>
__global__ void __launch_bounds__(256) sample_kernel(const T* __restrict__ logits, int64_t* __restrict__ out, int V,
                                                     int chunk, float inv_temp, uint32_t seed, uint32_t step,
                                                     int row0, const float* __restrict__ temps,
                                                     const int64_t* __restrict__ seeds,
                                                     const int32_t* __restrict__ steps,
                                                     float* __restrict__ g_samp_val, int* __restrict__ g_samp_idx) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const int lrow = blockIdx.y;
  const int64_t row = (int64_t)row0 + lrow;
  const T* x = logits + row * V;
  const int c0 = blockIdx.x * chunk, c1 = min(V, c0 + chunk);
  uint32_t nseed = seed + (uint32_t)row * 7919u;
  if (temps) {  // per-row parameters (sample_rows without top-k / top-p): noise of sampling.hip
    const float t = temps[row];
    inv_temp = t > 0.f ? 1.f / t : 0.f;
    nseed = (uint32_t)seeds[row];
    step = (uint32_t)steps[row];
  }
  float best = -INFINITY;
  int bi = c0 < V ? c0 : 0;
  for (int cb = c0 + (int)threadIdx.x; cb < c1; cb += 256 * 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {  // 8 independent loads in flight per thread
      const int c = cb + 256 * u;
      if constexpr (sizeof(T) == 2) v[u] = c < c1 ? bf2f(reinterpret_cast<const uint16_t*>(x)[c]) : -INFINITY;
      else v[u] = c < c1 ? reinterpret_cast<const float*>(x)[c] : -INFINITY;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int c = cb + 256 * u;
      if (c >= c1) break;
      float w = v[u];
      if (inv_temp > 0.f) w = w * inv_temp + gumbel_noise(nseed, step, (uint32_t)c);  // Gumbel-max
      if (w > best) { best = w; bi = c; }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) samp_pick(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
  if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) samp_pick(best, bi, sv[w], si[w]);
    g_samp_val[lrow * kSampMaxChunks + blockIdx.x] = best;
    g_samp_idx[lrow * kSampMaxChunks + blockIdx.x] = bi;
  }
}

// partials of one row (chunk order) -> out[row]; grid rows, one wave
__global__ void __launch_bounds__(64) sample_final_kernel(int64_t* __restrict__ out, int nch, int row0,
                                                          const float* __restrict__ g_samp_val,
                                                          const int* __restrict__ g_samp_idx) {
  const int lrow = blockIdx.x, l = threadIdx.x;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  if (l < nch) {
    best = g_samp_val[lrow * kSampMaxChunks + l];
    bi = g_samp_idx[lrow * kSampMaxChunks + l];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) samp_pick(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
  if (l == 0) out[(int64_t)row0 + lrow] = bi == 0x7fffffff ? 0 : bi;
}

}  // namespace mx

using namespace mx;

// bt / maxb: paged cache (block table [slots, maxb]; max_seq = the block size), nullptr: contiguous
extern "C" int mx_rope_append(const uint16_t* qkv, const float* cosb, const float* sinb, const int32_t* pos,
                              const int32_t* slots, uint16_t* q, uint16_t* kc, uint16_t* vc, int B, int Hq, int Hkv,
                              int D, int max_seq, const int32_t* bt, int maxb, hipStream_t stream) {
  const int64_t items = (int64_t)B * (Hq + 2 * Hkv) * (D / 16);
  if (items <= 0) return 0;
  const int grid = (int)std::min<int64_t>(1024, (items + 255) / 256);
#define RA(DD) \
  rope_append_kernel<DD><<<grid, 256, 0, stream>>>(qkv, cosb, sinb, pos, slots, q, kc, vc, B, Hq, Hkv, max_seq, bt, maxb)
  if (D == 128) RA(128); else if (D == 64) RA(64); else if (D == 32) RA(32); else return -1;
#undef RA
  return (int)hipGetLastError();
}

extern "C" int mx_decode_attn(const uint16_t* q, const uint16_t* kc, const uint16_t* vc, const int32_t* lens,
                              int len_off, const int32_t* slots, float* part_ml, float* part_o, uint16_t* out, int B,
                              int Hq, int Hkv, int D, int max_seq, int nsplit, float scale, const int32_t* bt,
                              int maxb, unsigned int* cnt, hipStream_t stream) {
  if (B <= 0) return 0;
  if (Hq % Hkv || Hq / Hkv > kMaxRep) return -1;
  if (bt && max_seq % kSplit) return -1;  // a split must lie inside one block
  dim3 grid(nsplit, Hkv, B);
  const float sl = scale * 1.4426950408889634f;
  if (D == 128) {  // out == nullptr: partials only (the o-projection merges them: skinny_gemm.hip MERGE)
    // cnt (zeroed [B * Hkv] counters, owned by the caller): the splits merge in-launch
    // MXLLM_DECODE_HANDOFF: hand-off protocol of the in-launch merge (see the kernel; read per call)
    const char* pe = getenv("MXLLM_DECODE_HANDOFF");
    const int proto = pe && *pe ? atoi(pe) : 4;
    const bool fused = out && cnt && proto >= 1 && proto <= 4;
    decode_attn_mfma_kernel<<<grid, 256, 0, stream>>>(q, kc, vc, lens, len_off, slots, part_ml, part_o, Hq, Hkv,
                                                      max_seq, nsplit, sl, bt, maxb, out, fused ? cnt : nullptr,
                                                      proto);
    if (out && !fused) decode_combine_kernel<128><<<B * Hq, 128, 0, stream>>>(part_ml, part_o, out, nsplit);
    return (int)hipGetLastError();
  }
  if (!out) return -1;
#define DA(DD)                                                                                                  \
  decode_attn_kernel<DD><<<grid, 256, 0, stream>>>(q, kc, vc, lens, len_off, slots, part_ml, part_o, Hq, Hkv, \
                                                   max_seq, nsplit, sl, bt, maxb);                              \
  decode_combine_kernel<DD><<<B * Hq, DD, 0, stream>>>(part_ml, part_o, out, nsplit)
  if (D == 64) { DA(64); } else if (D == 32) { DA(32); } else return -1;
#undef DA
  return (int)hipGetLastError();
}

// x [R, 128] bf16 rows (stride ldx, a multiple of 8) -> codes [R, 128] u8, scales [R] f32
extern "C" int mx_kv8_quant_rows(const uint16_t* x, int64_t ldx, uint8_t* q, float* s, int64_t R,
                                 hipStream_t stream) {
  if (R <= 0) return 0;
  if (ldx % 8 || ldx < 128 || (R + 15) / 16 > 0x7fffffff) return -1;
  kv8_quant_rows_kernel<<<(unsigned)((R + 15) / 16), 256, 0, stream>>>(x, ldx, q, s, R);
  return (int)hipGetLastError();
}

// mx_rope_append into kv8 pools (codes kq / vq, scales ks / vs); head_dim 128
extern "C" int mx_rope_append_kv8(const uint16_t* qkv, const float* cosb, const float* sinb, const int32_t* pos,
                                  const int32_t* slots, uint16_t* q, uint8_t* kq, float* ks, uint8_t* vq, float* vs,
                                  int B, int Hq, int Hkv, int max_seq, const int32_t* bt, int maxb,
                                  hipStream_t stream) {
  const int64_t items = (int64_t)B * (Hq + 2 * Hkv) * 8;
  if (items <= 0) return 0;
  if ((items + 255) / 256 > 0x7fffffff) return -1;
  rope_append_kv8_kernel<<<(unsigned)((items + 255) / 256), 256, 0, stream>>>(qkv, cosb, sinb, pos, slots, q, kq, ks,
                                                                              vq, vs, B, Hq, Hkv, max_seq, bt, maxb);
  return (int)hipGetLastError();
}

// mx_decode_attn over kv8 pools; head_dim 128, always the combine kernel
extern "C" int mx_decode_attn_kv8(const uint16_t* q, const uint8_t* kq, const float* ks, const uint8_t* vq,
                                  const float* vs, const int32_t* lens, int len_off, const int32_t* slots,
                                  float* part_ml, float* part_o, uint16_t* out, int B, int Hq, int Hkv, int max_seq,
                                  int nsplit, float scale, const int32_t* bt, int maxb, hipStream_t stream) {
  if (B <= 0) return 0;
  if (Hq % Hkv || Hq / Hkv > kMaxRep || !out) return -1;
  if (bt && max_seq % kSplit) return -1;  // a split must lie inside one block
  dim3 grid(nsplit, Hkv, B);
  decode_attn_kv8_kernel<<<grid, 256, 0, stream>>>(q, kq, ks, vq, vs, lens, len_off, slots, part_ml, part_o, Hq, Hkv,
                                                   max_seq, nsplit, scale * 1.4426950408889634f, bt, maxb);
  decode_combine_kernel<128><<<B * Hq, 128, 0, stream>>>(part_ml, part_o, out, nsplit);
  return (int)hipGetLastError();
}

// verify_attn over bf16 or kv8 pools (operand rules: mx::vf_takes, kernels/verify_args.h)
extern "C" int mx_verify_attn(const mx::VfLaunch& L, float scale, hipStream_t stream) {
  if (L.B <= 0) return 0;
  if (!vf_takes(L)) return -1;
  const dim3 grid((unsigned)L.nsplit, (unsigned)L.Hkv, (unsigned)L.B);
  const float sl = scale * 1.4426950408889634f;
  const bool two = L.n * (L.Hq / L.Hkv) > 16;
#define VA(KV, NB)                                                                                                   \
  verify_attn_kernel<KV, NB><<<grid, 256, 0, stream>>>(                                                              \
      (const uint16_t*)L.q, L.k_pool, L.k_scale, L.v_pool, L.v_scale, L.lens, L.nq, L.slots, L.part_ml, L.part_o,    \
      (int)L.Hq, (int)L.Hkv, (int)L.n, (int)L.max_seq, (int)L.nsplit, sl, L.bt, (int)L.maxb)
  if (L.kv_u8) {
    if (two) VA(KvFp8, 2); else VA(KvFp8, 1);
  } else {
    if (two) VA(KvBf16, 2); else VA(KvBf16, 1);
  }
#undef VA
  decode_combine_kernel<128><<<(unsigned)(L.B * L.n * L.Hq), 128, 0, stream>>>(L.part_ml, L.part_o, (uint16_t*)L.out,
                                                                               (int)L.nsplit);
  return (int)hipGetLastError();
}

// ws: float workspace of mx_sample_ws_floats(B) elements
extern "C" int64_t mx_sample_ws_floats(int B) {
  return 2 * (int64_t)std::min(B, kSampMaxRows) * kSampMaxChunks;
}

static int sample_launch(const void* logits, int is_bf16, int64_t* out, int B, int V, float temperature,
                         uint32_t seed, uint32_t step, const float* temps, const int64_t* seeds,
                         const int32_t* steps, float* ws, hipStream_t stream) {
  if (B <= 0) return 0;
  if (V <= 0 || !ws) return -1;
  float* pv = ws;
  int* pi = reinterpret_cast<int*>(ws + (int64_t)std::min(B, kSampMaxRows) * kSampMaxChunks);
  const float it = temperature > 0.f ? 1.f / temperature : 0.f;
  int chunk = 2048, nch = (V + chunk - 1) / chunk;
  if (nch > kSampMaxChunks) {
    chunk = ((V + kSampMaxChunks - 1) / kSampMaxChunks + 255) / 256 * 256;
    nch = (V + chunk - 1) / chunk;
  }
  for (int r0 = 0; r0 < B; r0 += kSampMaxRows) {
    const dim3 grid(nch, std::min(kSampMaxRows, B - r0));
    if (is_bf16)
      sample_kernel<uint16_t><<<grid, 256, 0, stream>>>((const uint16_t*)logits, out, V, chunk, it, seed, step, r0,
                                                         temps, seeds, steps, pv, pi);
    else
      sample_kernel<float><<<grid, 256, 0, stream>>>((const float*)logits, out, V, chunk, it, seed, step, r0, temps,
                                                      seeds, steps, pv, pi);
    sample_final_kernel<<<grid.y, 64, 0, stream>>>(out, nch, r0, pv, pi);
  }
  return (int)hipGetLastError();
}

extern "C" int mx_sample(const void* logits, int is_bf16, int64_t* out, int B, int V, float temperature,
                         uint32_t seed, uint32_t step, float* ws, hipStream_t stream) {
  return sample_launch(logits, is_bf16, out, B, V, temperature, seed, step, nullptr, nullptr, nullptr, ws, stream);
}

// per-row temperature (<= 0: greedy), seed and step, no top-k / top-p: the draws of
// sampling.hip's sample_topkp_kernel for such rows (same noise), split over the vocabulary
extern "C" int mx_sample_temp_rows(const void* logits, int is_bf16, int64_t* out, int B, int V, const float* temps,
                                   const int64_t* seeds, const int32_t* steps, float* ws, hipStream_t stream) {
  return sample_launch(logits, is_bf16, out, B, V, 0.f, 0u, 0u, temps, seeds, steps, ws, stream);
}
