// Host-side description of a document-masked training attention launch (attn_doc.hip), forward or
// backward, and THE check that says whether it is taken.  Plain C++: no HIP, no torch -- the launcher,
// the torch binding and the stand-alone test (tests/native/test_attn_doc_args.cpp) include this one file.
// The launcher asks the check before it enqueues anything, so a refusal (-1) always means "nothing
// launched, nothing written".
//
// Self-attention over packed documents: query i sees key j iff doc_start[b, i] <= j <= i.
// Layouts as attn_args.h: q [B,Hq,S,D], k/v [B,Hkv,S,D] bf16 head-major; o token-major [B,S,Hq*D] bf16
// rows with row stride ldo; dout [B,S,Hq*D] bf16 contiguous; lse, delta [B,Hq,S] f32 (lse in the log2
// domain); doc_start, doc_end [B,S] int32 (doc_end exclusive).  The backward is the split structure
// only: dS^T (bf16) through the `work` image of ab_work_bytes mode 3, f32 dQ [B,Hq,S,D] and one f32
// dK / dV partial per q head [B,Hq,S,D] (a KV head's partials consecutive), as rope_merge_bwd reads them.
//
// THE dS^T INVARIANT.  The image is not zeroed.  The key-block kernel of 128-key block kb writes the
// pieces (kb, t) for the 64-row q tiles t = 2 kb .. (doc_end[b, min(128 kb + 127, S - 1)] - 1) / 64;
// the dQ kernel of q tile t reads the pieces (kb, t) for kb = doc_start[b, 64 t] / 128 .. t / 2.  The
// read range lies inside the write range: the last key of every block read is at or after doc_start of
// the tile's first row, so it lies in that row's document or a later one, which ends past that row.
// Both kernels clamp what they derive from the tables (keys to [0, q], q tiles to [diagonal, S)), and
// the dQ kernel clamps every piece it fetches into its tile's read range: a malformed table gives wrong
// numbers, never an access outside the sequence.
#pragma once
#include <stdint.h>

#include "attn_args.h"

namespace mx {

struct AdLaunch {
  int bwd;  // 0 = forward (q, k, v, doc_start -> o, lse), 1 = backward
  const void* q;
  const void* k;
  const void* v;
  const void* doc_start;
  const void* doc_end;  // backward only
  void* o;              // forward: written; backward: read
  void* lse;            // forward: written; backward: read
  const void* dout;     // backward
  void* delta;          // backward workspace [B,Hq,S] f32
  void* dq;             // [B,Hq,S,D] f32
  void* dkp;            // [B,Hq,S,D] f32
  void* dvp;
  void* work;           // ad_work_bytes(L) bytes, no zeroing
  int q_bf16, kv_bf16, o_bf16, lse_f32, doc_i32;
  int dout_bf16, out_f32;  // backward
  int64_t B, Hq, Hkv, S, D;
  int64_t ldo;  // elements
};

// bytes of `work`: the dS^T image of the plain split backward
inline int64_t ad_work_bytes(const AdLaunch& L) { return L.B * L.Hq * ab_ds_bytes_per_head(L.S, L.S); }

// Empty calls are taken and launch nothing.
inline bool ad_empty(const AdLaunch& L) { return L.B <= 0 || L.S <= 0; }

// Whether the launch is taken: the rules of af_takes / ab_takes (split mode, causal self-attention) on
// the same numbers, and the tables.
inline bool ad_takes(const AdLaunch& L) {
  if (L.bwd != 0 && L.bwd != 1) return false;
  if (ad_empty(L)) return true;
  if (!L.doc_start || !L.doc_i32) return false;
  if (!L.bwd) {
    AfLaunch F{L.q, L.k, L.v, L.o, L.lse, L.q_bf16, L.kv_bf16, L.o_bf16, L.lse_f32, L.B, L.Hq, L.Hkv, L.S, L.S, L.D,
               L.ldo, 1};
    return af_takes(F);
  }
  if (!L.doc_end) return false;
  AbLaunch A{};
  A.q = L.q, A.k = L.k, A.v = L.v, A.o = L.o, A.dout = L.dout, A.lse = L.lse;
  A.delta = L.delta, A.dq = L.dq, A.dkp = L.dkp, A.dvp = L.dvp, A.work = L.work;
  A.q_bf16 = L.q_bf16, A.kv_bf16 = L.kv_bf16, A.o_bf16 = L.o_bf16, A.dout_bf16 = L.dout_bf16;
  A.lse_f32 = L.lse_f32, A.out_f32 = L.out_f32;
  A.B = L.B, A.Hq = L.Hq, A.Hkv = L.Hkv, A.S = A.Sk = L.S, A.D = L.D, A.ldo = L.ldo;
  A.causal = 1, A.dq_mode = 3, A.hpw = 1;
  return ab_takes(A);
}

}  // namespace mx
