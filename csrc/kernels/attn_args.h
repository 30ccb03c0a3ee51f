// Host-side description of a training attention launch -- forward (attn_fwd.hip) and backward
// (attn_bwd.hip) -- and THE check of each that says whether the launch is taken.  Plain C++: no HIP, no
// torch -- the launchers, the torch binding and the stand-alone test (tests/native/test_attn_args.cpp)
// include this one file.  A launcher asks its check before it enqueues anything, so a refusal (-1)
// always means "nothing launched, nothing written".  The workspace and partial-head arithmetic of the
// backward is stated here once; the header reads no environment.
//
// Layouts: q [B,Hq,S,D], k/v [B,Hkv,Sk,D] bf16 head-major; o token-major [B,S,Hq*D] bf16 rows with row
// stride ldo; dout [B,S,Hq*D] bf16 contiguous; lse, delta [B,Hq,S] f32.
#pragma once
#include <stdint.h>

namespace mx {

struct AfLaunch {
  const void* q;
  const void* k;
  const void* v;
  void* o;
  void* lse;
  int q_bf16, kv_bf16, o_bf16, lse_f32;  // element types of q, of k and v, of o, of lse
  int64_t B, Hq, Hkv, S, Sk, D;
  int64_t ldo;  // elements
  int causal;   // 0 / 1; keys 0 .. q + Sk - S visible to query q
};

struct AbLaunch {
  const void* q;
  const void* k;
  const void* v;
  const void* o;
  const void* dout;
  const void* lse;
  void* delta;  // workspace [B,Hq,S] f32
  void* dq;     // mode 1: [B,Hq,ab_s_pad(S),D] f32, ZEROED (the padded rows absorb the unguarded tail
                // atomics); modes 2, 3: [B,Hq,S,D] f32, not read; unused (may be null) with dqkv
  void* dkp;    // dK / dV partials [B, Hq / hpw, Sk, D] f32: each KV head's partials are consecutive
  void* dvp;
  void* work;   // modes 2, 3: ab_work_bytes(L) bytes, no zeroing
  void* dqkv;   // optional (mode 3, D = 128, Sk = S): token-major d(qkv) bf16 rows of stride ldq; the dQ
                // kernel writes the q columns with the inverse RoPE applied, and no f32 dq at all
  const void* cos;  // with dqkv: RoPE tables [cos_rows, D/2] f32
  const void* sin;
  int q_bf16, kv_bf16, o_bf16, dout_bf16, lse_f32;
  int out_f32;    // delta, dq, dkp and dvp are f32
  int dqkv_bf16;  // with dqkv: it is bf16 and cos / sin are f32
  int64_t B, Hq, Hkv, S, Sk, D;
  int64_t ldo, ldq, cos_rows;
  int causal;
  int dq_mode;  // 1 = f32 atomics, 2 = per-key-block partials + ordered reduce, 3 = split (dS^T through
                // `work`, dQ by attn_bwd_dq_kernel; deterministic, default)
  int64_t hpw;  // q-heads one workgroup of the 8-wave key-block kernel sums (ab_hpw), 1 elsewhere
};

// dq / dS^T rows are padded to whole 64-row q tiles
inline int64_t ab_s_pad(int64_t S) { return (S + 63) / 64 * 64; }
// 128-key blocks: the key-block kernels' grid, and dS^T holds ab_key_blocks(Sk) * 128 key rows
inline int64_t ab_key_blocks(int64_t Sk) { return (Sk + 127) / 128; }
// dS^T image of one q head (mode 3), bytes
inline int64_t ab_ds_bytes_per_head(int64_t S, int64_t Sk) { return ab_key_blocks(Sk) * 128 * ab_s_pad(S) * 2; }
// bytes of `work` (0 for mode 1), for a launch ab_shape_takes admits.  Mode 2: one f32 dQ partial
// [B,Hq,S_pad,D] per key block; mode 3: the bf16 dS^T image [B*Hq, S_pad/64, key rows, 64].
inline int64_t ab_work_bytes(const AbLaunch& L) {
  if (L.dq_mode == 2) return ab_key_blocks(L.Sk) * L.B * L.Hq * ab_s_pad(L.S) * L.D * 4;
  if (L.dq_mode == 3) return L.B * L.Hq * ab_ds_bytes_per_head(L.S, L.Sk);
  return 0;
}
// The backward that writes d(qkv) itself (dqkv): split mode, D = 128, self-attention
inline bool ab_takes_rope(int64_t dq_mode, int64_t D, int64_t S, int64_t Sk) {
  return dq_mode == 3 && D == 128 && Sk == S;
}
// q-heads per workgroup of the 8-wave key-block kernel (split mode, D = 128, bwd8_on): the largest of
// 4 / 2 that divides the GQA group and still leaves >= 512 workgroups (2 per CU) for the causal
// heavy-to-light balance, else 1; forced > 0 picks a value (1 if it does not divide the group).  1 on
// every other path.
inline int64_t ab_hpw(int64_t B, int64_t Hq, int64_t Hkv, int64_t Sk, int64_t D, int64_t dq_mode, bool bwd8_on,
                      int64_t forced) {
  if (dq_mode != 3 || D != 128 || !bwd8_on || Hq <= 0 || Hkv <= 0 || Hq % Hkv) return 1;
  const int64_t G = Hq / Hkv, nkb = ab_key_blocks(Sk);
  if (forced > 0) return G % forced == 0 ? forced : 1;
  for (int64_t hpw = 4; hpw > 1; hpw >>= 1) {
    const int64_t HP = Hq / hpw;
    // nkb * B * HP >= 512 (a factor of 512 or more first: the product of three smaller ones fits)
    if (G % hpw == 0 && (nkb >= 512 || B >= 512 || HP >= 512 || nkb * B * HP >= 512)) return hpw;
  }
  return 1;
}
// dK / dV partial heads per batch row
inline int64_t ab_partial_heads(int64_t B, int64_t Hq, int64_t Hkv, int64_t Sk, int64_t D, int64_t dq_mode,
                                bool bwd8_on, int64_t forced) {
  return Hq / ab_hpw(B, Hq, Hkv, Sk, D, dq_mode, bwd8_on, forced);
}

// Empty calls are taken and launch nothing (the forward with no keys still writes o = 0).
inline bool af_empty(const AfLaunch& L) { return L.B <= 0 || L.S <= 0; }
inline bool ab_empty(const AbLaunch& L) { return L.B <= 0 || L.S <= 0 || L.Sk <= 0; }

namespace attn_detail {
constexpr int64_t I32 = 0x7fffffff;
// a * b * c <= lim for positive factors, as divisions (the product itself may not fit 64 bits)
inline bool prod_le(int64_t a, int64_t b, int64_t c, int64_t lim) { return a <= lim / b && a * b <= lim / c; }
// the shape rules both directions share
inline bool heads_ok(int64_t Hq, int64_t Hkv, int64_t D, int64_t ldo, int causal) {
  // GQA: whole groups of q-heads per KV head
  if (Hq <= 0 || Hkv <= 0 || Hq % Hkv) return false;
  // the MFMA tilings
  if (D != 32 && D != 64 && D != 128) return false;
  if (Hq > I32 / D) return false;  // Hq * D, the token row, in 31 bits (and the products below in 64)
  // o rows hold every head; 16-B loads / 8-B stores of them
  if (ldo < Hq * D || ldo % 8) return false;
  return causal == 0 || causal == 1;
}
}  // namespace attn_detail

// Whether the forward launch is taken.
inline bool af_takes(const AfLaunch& L) {
  using namespace attn_detail;
  if (af_empty(L)) return true;
  if (!L.q || !L.k || !L.v || !L.o || !L.lse) return false;
  if (!L.q_bf16 || !L.kv_bf16 || !L.o_bf16 || !L.lse_f32) return false;
  if (L.Sk < 0 || !heads_ok(L.Hq, L.Hkv, L.D, L.ldo, L.causal)) return false;
  // 32-bit quantities of attn_fwd_kernel and its launch (as divisions: the products may not fit 64 bits)
  if (L.ldo > I32) return false;                         // ldo is an int argument
  if (L.S > I32 - 127) return false;                     // S + 127, the q-block round-up
  if (!prod_le(L.B, L.Hq, L.S, I32)) return false;       // (b * Hq + h) * S, the q / lse row (the grid,
                                                         // q-blocks * B * Hq, is no larger)
  if (L.Sk > I32 / (2 * L.D) - 64) return false;         // (Sk + 64) * 2 D: byte offsets into one head's K / V
                                                         // (the descriptor's range; the last tile's end)
  if (L.Sk > 0 && !prod_le(L.B, L.Hkv, L.Sk, I32)) return false;  // (b * Hkv + hk) * Sk, the K / V row
  return true;
}

// The rules of the backward on numbers alone (the binding asks before it sizes the workspaces).
inline bool ab_shape_takes(const AbLaunch& L) {
  using namespace attn_detail;
  if (ab_empty(L)) return true;
  if (!heads_ok(L.Hq, L.Hkv, L.D, L.ldo, L.causal)) return false;
  if (L.dq_mode < 1 || L.dq_mode > 3) return false;
  // hpw: q-heads of one KV group; above 1 only where the 8-wave kernel runs
  if (L.hpw < 1 || (L.Hq / L.Hkv) % L.hpw || (L.hpw > 1 && (L.dq_mode != 3 || L.D != 128))) return false;
  // 32-bit quantities of the kernels and their launches (as divisions)
  if (L.S > I32 / (2 * L.D) - 64) return false;           // S_pad * 2 D: byte offsets into one head's Q
  if (L.Sk > I32 / (2 * L.D) - 128) return false;         // nkb * 128 * 2 D: byte offsets into one head's K / V,
                                                          // nkb * 128 the dS^T key rows
  const int64_t nkb = ab_key_blocks(L.Sk);
  if (!prod_le(ab_s_pad(L.S), L.Hq, 2 * L.D, I32)) return false;  // S_pad * Hq * D * 2: byte offsets into one
                                                                  // sequence's dout (and its record size)
  if (L.dq_mode != 3 && ab_s_pad(L.S) > I32 / (4 * L.D)) return false;  // S_pad * D * 4: byte offsets into one
                                                                        // head's f32 dQ (modes 1, 2)
  if (!prod_le(L.B, L.Hq, ab_s_pad(L.S), I32)) return false;  // B * Hq * S_pad rows: the delta / reduce / dQ grids
                                                              // (and ab_work_bytes stays far inside 64 bits)
  if (!prod_le(L.B, L.Hq, nkb, I32)) return false;        // the key-block grid: nkb * B * Hq
  if (!prod_le(L.B, L.Hkv, L.Sk, I32)) return false;      // (b * Hkv + hk) * Sk, the forward's K / V row
  return true;
}

// Whether the backward launch is taken.
inline bool ab_takes(const AbLaunch& L) {
  if (ab_empty(L)) return true;
  if (!L.q || !L.k || !L.v || !L.o || !L.dout || !L.lse || !L.delta || !L.dkp || !L.dvp) return false;
  if (!L.dq && !L.dqkv) return false;
  if (!L.q_bf16 || !L.kv_bf16 || !L.o_bf16 || !L.dout_bf16 || !L.lse_f32 || !L.out_f32) return false;
  if (!ab_shape_takes(L)) return false;
  if (L.dq_mode > 1 && !L.work) return false;
  // dqkv: the split dQ kernel writes d(q) with the inverse RoPE into it
  if (L.dqkv) {
    if (!ab_takes_rope(L.dq_mode, L.D, L.S, L.Sk) || !L.cos || !L.sin || !L.dqkv_bf16) return false;
    if (L.ldq % 8 || L.ldq < L.Hq * L.D) return false;  // 16-B stores into rows that hold the q columns
    if (L.cos_rows < L.S) return false;                 // a table row per position
  }
  return true;
}

}  // namespace mx
