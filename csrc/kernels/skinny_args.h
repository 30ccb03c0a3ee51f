// Host-side description of a skinny decode GEMM launch (skinny_gemm.hip, and mx_w8a16_gemm of
// fp8_gemm.hip) and THE check that says whether a launch is taken.  Plain C++: no HIP, no torch --
// the launchers, the torch bindings and the stand-alone test (tests/native/test_skinny_args.cpp)
// include this one file, and mxllm/ops/linear.py `sk_takes` mirrors `mx::sk_takes` line by line
// (tests/test_skinny_args.py runs both over one grid).  Every launcher calls sk_takes before it
// enqueues anything, so a refusal (-1) always means "nothing launched".
#pragma once
#include <stdint.h>

namespace mx {

// kernel arguments of the fused prologues / epilogues (device code: decode_fuse.h)
struct SkNorm {
  const uint16_t* delta;  // [M, K] sub-block output added to the residual (nullptr: plain RMSNorm)
  int64_t ldd;
  const uint16_t* gamma;  // [K]
  uint16_t* h_out;        // [M, K] (row stride K): h + delta, written by workgroup 0
  float eps;
};

struct SkRope {
  const float* cosb;     // [max_pos, 64]
  const float* sinb;
  const int32_t* pos;    // [M] position of the new token
  const int32_t* slots;  // [M] cache slot (nullptr: row index)
  uint16_t* q;           // [M, Hq, 128]
  uint16_t* kc;          // [slots, Hkv, max_seq, 128], or paged [blocks, Hkv, block, 128]
  uint16_t* vc;
  int Hq, Hkv, max_seq;  // max_seq: the cache's sequence dimension (the block size when paged)
  const int32_t* bt;     // paged: block table [slots, maxb] (nullptr: contiguous)
  int maxb;
};

// split-K decode attention partials (decode.hip): ml [M, Hq, nsplit, 2], po [M, Hq, nsplit, 128]
struct SkMerge {
  const float* ml;
  const float* po;
  int nsplit;
};

enum SkEntry : int {
  SK_PLAIN = 0,   // Y [M, N] = X . W^T
  SK_SWIGLU = 1,  // Y [M, N/2] = silu(g) * u, W = [gate; up] [N, K]
  SK_NORM = 2,    // X = rmsnorm(h [+ delta]) in the prologue (na); `swiglu`: the SWIGLU epilogue
  SK_ROPE = 3,    // RoPE + KV-cache append in the epilogue (rp), no Y; `norm`: the NORM prologue
  SK_MERGE = 4,   // X [M, K = Hq * 128] = the merged split partials (mg), no X operand
  SK_W8 = 5,      // mx_w8a16_gemm: W e4m3 codes [N, K] (contiguous rows), `scale` [N]
};

struct SkMat {  // one operand: base, row stride in elements
  const void* p;
  int64_t ld;
};

struct SkLaunch {
  SkEntry entry;
  SkMat X, W, Y;  // X [M, K] (NORM / ROPE: the residual h), W [N, K], Y [M, N or N/2]
  int M, N, K;
  int swiglu, norm;
  SkNorm na;
  SkRope rp;
  SkMerge mg;
  const float* scale;
};

// Whether the launch is taken (M >= 1: the launchers return 0 for M <= 0 before they ask).  The
// rules are the former launchers' guards, kept as they were, plus: what is dereferenced is not null.
inline bool sk_takes(const SkLaunch& L) {
  const int64_t M = L.M, N = L.N, K = L.K, ldx = L.X.ld, ldw = L.W.ld, ldy = L.Y.ld;
  const bool rope = L.entry == SK_ROPE, merge = L.entry == SK_MERGE, w8 = L.entry == SK_W8;
  const bool norm = L.entry == SK_NORM || (rope && L.norm);  // X rows built in LDS by the RMSNorm
  const bool swiglu = L.entry == SK_SWIGLU || (L.entry == SK_NORM && L.swiglu);
  if (L.entry < SK_PLAIN || L.entry > SK_W8) return false;
  if (!L.W.p || (!merge && !L.X.p) || (!rope && !L.Y.p)) return false;
  // each wave's eighth of K is whole 64-k chunks; one or two 16-token blocks, under a prologue
  // 4 rows whose M * K * 2 bytes fit the 64 KiB of LDS
  if (K % 512 || M > (norm || merge ? 4 : rope ? 16 : 32) || ((norm || merge) && M * K > 32768)) return false;
  // 16-B row loads of X and W, rows at least K long (MERGE: no X operand; W8: contiguous code rows)
  if (!merge && (ldx % 8 || ldx < K)) return false;
  if (!w8 && (ldw % 8 || ldw < K)) return false;
  // 16 channels per workgroup, 8-B stores into Y rows that hold the output (SWIGLU: N / 2 wide)
  if (!rope && (N % 16 || ldy % 4 || ldy < (swiglu ? N / 2 : N))) return false;
  // delta rows: 16-B loads (prologue or not); with delta the prologue also stores h + delta
  if ((L.entry == SK_NORM || rope) && L.na.ldd % 8) return false;
  if (norm && (!L.na.gamma || (L.na.delta && (L.na.ldd < K || !L.na.h_out)))) return false;
  if (rope) {
    const SkRope& r = L.rp;
    if (r.Hq <= 0 || r.Hkv <= 0 || r.max_seq <= 0 || N != ((int64_t)r.Hq + 2 * (int64_t)r.Hkv) * 128) return false;
    if (!r.cosb || !r.sinb || !r.pos || !r.q || !r.kc || !r.vc || (r.bt && r.maxb <= 0)) return false;
  }
  if (merge && (!L.mg.ml || !L.mg.po || L.mg.nsplit < 1)) return false;
  return !w8 || L.scale;
}

}  // namespace mx
