// Host-side description of a gemm8 launch (csrc/kernels/gemm8.hip) and THE check that says whether
// a launch is taken.  Plain C++: no HIP, no torch -- the launchers, the torch bindings and the
// stand-alone test (tests/native/test_gemm8_args.cpp) all include this one file, and
// mxllm/ops/gemm.py `g8_takes` mirrors `mx::g8_takes` line by line (tests/test_gemm8_args.py runs
// both over one grid).  Every launcher calls g8_takes before it enqueues anything, so a refusal
// (-1) always means "nothing launched".
#pragma once
#include <stdint.h>

namespace mx {

// epilogue of gemm8_kernel (the EPI template argument; documented at the top of gemm8.hip)
enum G8EpiMode : int { G8_EPI_NONE = 0, G8_EPI_ROPE = 1, G8_EPI_SWIGLU = 2, G8_EPI_SWIGLU_BWD = 3 };

struct G8Epi {
  uint16_t* q;        // ROPE: [B, Hq, S, 128]
  uint16_t* k;        //       [B, Hkv, S, 128]
  uint16_t* v;        //       [B, Hkv, S, 128]
  const float* cosb;  //       [>= S, 64] f32 (host table, mxllm/ops/reference.py rope_tables)
  const float* sinb;
  int S, Hq, Hkv;
  uint16_t* m;        // SWIGLU: [T, F] with row stride ldm (SWIGLU_BWD: optional recomputed m)
  int64_t ldm;
  int F;
  const uint16_t* gu; // SWIGLU_BWD: the forward's [T, 2F] with row stride ldg
  int64_t ldg;
  float* sq;          // plain bf16 beta-0 output: per-tile sum of squares of the stored values
};

// the C entry point a description is for (csrc/bindings.h)
enum G8Entry : int {
  G8_PLAIN = 0,      // mx_gemm8
  G8_SQ = 1,         // mx_gemm8_sq
  G8_EPI = 2,        // mx_gemm8_epi (epi = ROPE / SWIGLU / SWIGLU_BWD)
  G8_TAIL = 3,       // mx_gemm8_tail
  G8_ROPE_TAIL = 4,  // mx_gemm8_rope_tail (epi = ROPE)
};

// one operand: base, row stride in elements, storage order (kc: k-contiguous rows; C: always 1)
struct G8Mat {
  const void* p;
  int64_t ld;
  int kc;
};

struct G8Launch {
  G8Entry entry;
  G8Mat A, B, C;  // A [M][K] when kc else [K][M]; B [N][K] when kc else [K][N]; C [M][ldc]
  int M, N, K;
  int out_f32;    // C fp32 (else bf16)
  float beta;     // 0 or 1
  int epi;        // G8EpiMode
  G8Epi ep;
  int rows, at;   // tail launches: split at column `at` (row when `rows`)
  const void* ws; // tail launches: the two fp32 half-K images
  int ph;         // schedule asked for (8, 4; 5 = 4-phase persistent)
  const float* alpha_t;  // alpha = alpha_f * (*alpha_t when set, on the device); not part of the check
  float alpha_f;
};

constexpr int G8_BK = 64;

inline bool g8_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
// rows * ld elements of bf16 stay under 2^31 bytes (the 32-bit buffer-descriptor offsets); ld > 0
inline bool g8_span_ok(int64_t rows, int64_t ld) {
  const int64_t lim = (int64_t)1 << 30;
  return ld < lim && rows * ld < lim;  // rows <= 2^31 and ld < 2^30: no overflow
}

// Whether the launch is taken.  Rules shared by every entry point first, then one block per entry
// point / epilogue; the per-entry differences are the parent launchers', kept as they were.
inline bool g8_takes(const G8Launch& L) {
  const int M = L.M, N = L.N, K = L.K, epi = L.epi;
  const bool a_kc = L.A.kc != 0, b_kc = L.B.kc != 0;
  const int64_t lda = L.A.ld, ldb = L.B.ld, ldc = L.C.ld;
  const bool tail = L.entry == G8_TAIL || L.entry == G8_ROPE_TAIL;
  const bool rope = (L.entry == G8_EPI || L.entry == G8_ROPE_TAIL) && epi == G8_EPI_ROPE;
  const bool swiglu = L.entry == G8_EPI && epi == G8_EPI_SWIGLU;
  const bool swiglu_bwd = L.entry == G8_EPI && epi == G8_EPI_SWIGLU_BWD;
  // entry point <-> epilogue and operand orders: fused forward epilogues are TN, SWIGLU_BWD is NN
  if (L.entry == G8_EPI || L.entry == G8_ROPE_TAIL) {
    if (!(rope || swiglu || swiglu_bwd) || !a_kc || b_kc != !swiglu_bwd) return false;
  } else if (epi != G8_EPI_NONE) {
    return false;
  }
  // whole 256 x 256 tiles (a tail launch's plain and split parts are whole tiles too)
  if (M <= 0 || N <= 0 || K <= 0 || (M & 255) || (N & 255)) return false;
  // a k-contiguous operand is staged in whole K-tiles (mn-contiguous rows past K read as zeros)
  if ((a_kc || b_kc) && K % G8_BK) return false;
  // 16-B rows on 16-B bases, rows at least as long as what is stored in them
  if (lda % 8 || ldb % 8 || !g8_al16(L.A.p) || !g8_al16(L.B.p)) return false;
  if (lda < (a_kc ? K : M) || ldb < (b_kc ? K : N)) return false;
  // operand spans under 2^31 bytes: 256 rows of a k-contiguous operand (the descriptor is based at
  // the tile's first row), all K-tile-padded rows of an mn-contiguous one (SWIGLU_BWD's W_down: K * ldb)
  // ... except the fused TN epilogues, which gather weight rows from the WHOLE matrix: N * ldb
  const int64_t kpad = ((int64_t)K + G8_BK - 1) / G8_BK * G8_BK;
  if (!g8_span_ok(a_kc ? 256 : kpad, lda)) return false;
  if (!g8_span_ok(b_kc ? (rope || swiglu ? (int64_t)N : 256) : kpad, ldb)) return false;
  if (L.beta != 0.f && L.beta != 1.f) return false;
  // C (ROPE writes q / k / v instead): 16-B base; bf16 rows are stored 16 B at a time (ldc % 8),
  // fp32 rows 16 B = 4 elements (ldc % 4); SWIGLU_BWD writes dgu, 2N wide
  if (!rope) {
    if (!g8_al16(L.C.p) || ldc % (L.out_f32 ? 4 : 8) || ldc < (swiglu_bwd ? 2 * (int64_t)N : (int64_t)N)) return false;
  }
  // per-tile sums of squares: mx_gemm8_sq needs the buffer; mx_gemm8_tail writes them only on the
  // 4-phase schedule (whole tiles: above)
  if (L.entry == G8_SQ && !L.ep.sq) return false;
  if (L.entry == G8_TAIL && L.ep.sq && L.ph != 4) return false;
  if (tail) {
    // both halves of K hold at least one K-tile; `at` and the rest are whole tiles; 16-B workspace
    const int rest = (L.rows ? M : N) - L.at;
    if (K < 2 * G8_BK || L.at <= 0 || rest <= 0 || (L.at & 255) || (rest & 255) || !g8_al16(L.ws)) return false;
    // (the split part's operand bases A + at * lda / B + at stay 16-B aligned: at % 256, ld % 8)
  }
  if (rope) {
    const G8Epi& e = L.ep;
    if (N != ((int64_t)e.Hq + 2 * (int64_t)e.Hkv) * 128 || e.S <= 0 || e.S % 256 || M % e.S) return false;
    if (!e.q || !e.k || !e.v || !e.cosb || !e.sinb || !g8_al16(e.q) || !g8_al16(e.k) || !g8_al16(e.v)) return false;
    // only the tail's sum pass reads the tables 16 B at a time
    if (L.entry == G8_ROPE_TAIL && (!g8_al16(e.cosb) || !g8_al16(e.sinb))) return false;
  }
  if (swiglu) {  // N = 2F, a tile = 128 gate + 128 up columns; gu -> C [M][>= 2F], m -> ep.m [M][>= F]
    if ((N / 2) % 128 || !L.C.p || !L.ep.m || L.ep.ldm < N / 2 || L.ep.ldm % 8 || !g8_al16(L.ep.m)) return false;
  }
  if (swiglu_bwd) {  // F = N; gu [M][>= 2F] read, dgu -> C, optional m [M][>= F]
    const G8Epi& e = L.ep;
    if (!L.C.p || !e.gu || e.ldg < 2 * (int64_t)N || e.ldg % 8 || !g8_al16(e.gu)) return false;
    if (e.m && (e.ldm < N || e.ldm % 8 || !g8_al16(e.m))) return false;
  }
  return true;
}

}  // namespace mx
