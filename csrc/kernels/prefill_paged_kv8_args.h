// Host-side description of a paged-KV prefill attention launch over the fp8 (kv8) cache
// (prefill_paged_kv8.hip) and THE check that says whether the launch is taken.  Plain C++: no HIP, no
// torch -- the launcher, the torch binding and the stand-alone test
// (tests/native/test_prefill_paged_kv8_args.cpp) include this one file.  Segments, the work table and every
// rule about them are prefill_paged_args.h's: pp8_takes asks pp_takes with the code pools in the place of
// the bf16 pools and adds the rules of the four-pool format.  A refusal (-1) means "nothing launched".
#pragma once
#include "prefill_paged_args.h"

namespace mx {

// One pool as the caller holds it: the check compares shapes, so the description carries them.
struct Pp8Pool {
  const void* p;
  int dtype_ok;    // codes: uint8, scales: float32
  int contiguous;
  int ndim;        // codes: 4 [blocks, Hkv, blk, D], scales: 3 [blocks, Hkv, blk]
  int64_t dim[4];
};

struct PpKv8Launch {
  const void* q;          // [T, Hq, D] token-major bf16
  Pp8Pool k_codes, k_scale, v_codes, v_scale;
  void* o;                // [T, ldo] token-major, ldo >= Hq * D
  const int32_t* bt;      // device: block table [slots, maxb]
  const int32_t* segs;    // device: [nseg, 4] = (row0, n, slot, p0)
  const int32_t* work;    // device: [nwork, 2] = (segment, q-block), heaviest first (pp_fill_work)
  const PpSeg* segs_host; // the host copy of `segs` that the check reads
  int q_bf16, o_bf16;
  int64_t T, Hq, D;       // Hkv, blocks and blk are the K code pool's dim[1], dim[0], dim[2]
  int64_t slots, maxb;
  int64_t nseg, nwork, ldo;
};

// The bf16 launch description with the code pools standing in for the bf16 pools: pp_takes' rules
// (head_dim, GQA, blk % 256, the 32-bit ranges -- a code row is half a bf16 row, so its byte offsets fit
// wherever the bf16 ones do -- and the segments) apply to it unchanged.
inline PpLaunch pp8_as_pp(const PpKv8Launch& L) {
  PpLaunch B{};
  B.q = L.q, B.k_pool = L.k_codes.p, B.v_pool = L.v_codes.p, B.o = L.o;
  B.bt = L.bt, B.segs = L.segs, B.work = L.work, B.segs_host = L.segs_host;
  B.q_bf16 = L.q_bf16, B.kv_bf16 = 1, B.o_bf16 = L.o_bf16;
  B.T = L.T, B.Hq = L.Hq, B.Hkv = L.k_codes.dim[1], B.D = L.D;
  B.blocks = L.k_codes.dim[0], B.blk = L.k_codes.dim[2], B.slots = L.slots, B.maxb = L.maxb;
  B.nseg = L.nseg, B.nwork = L.nwork, B.ldo = L.ldo;
  return B;
}

inline bool pp8_takes(const PpKv8Launch& L) {
  const Pp8Pool* codes[2] = {&L.k_codes, &L.v_codes};
  const Pp8Pool* scales[2] = {&L.k_scale, &L.v_scale};
  for (int i = 0; i < 2; ++i) {
    const Pp8Pool &c = *codes[i], &s = *scales[i];
    // code pools uint8 [blocks, Hkv, blk, D], scale pools float32, both contiguous
    if (!c.p || !s.p || !c.dtype_ok || !s.dtype_ok || !c.contiguous || !s.contiguous) return false;
    if (c.ndim != 4 || s.ndim != 3 || c.dim[3] != L.D) return false;
    // a scale per code row: the scale pool's shape is the code pool's without the last dimension
    // (the kernel addresses both with one row index)
    for (int d = 0; d < 3; ++d)
      if (s.dim[d] != c.dim[d]) return false;
    // K and V pools of one shape (one block id and one row offset serve both)
    for (int d = 0; d < 4; ++d)
      if (c.dim[d] != L.k_codes.dim[d]) return false;
  }
  return pp_takes(pp8_as_pp(L));
}

}  // namespace mx
