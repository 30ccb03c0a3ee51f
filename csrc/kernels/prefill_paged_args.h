// Host-side description of a paged-KV prefill attention launch (prefill_paged.hip) and THE check that
// says whether the launch is taken.  Plain C++: no HIP, no torch -- the launcher, the torch binding and
// the stand-alone test (tests/native/test_prefill_paged_args.cpp) include this one file.  The launcher
// calls pp_takes before it enqueues anything, so a refusal (-1) always means "nothing launched, nothing
// written".  The segment table comes from host lists, so the check reads the host copy.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

namespace mx {

constexpr int PP_BM = 128;  // query rows per workgroup
constexpr int PP_BN = 64;   // keys per tile

// One query segment: rows [row0, row0 + n) of q are positions [p0, p0 + n) of cache slot `slot`;
// row t sees keys 0 .. p0 + t of that slot.
struct PpSeg {
  int32_t row0, n, slot, p0;
};

struct PpLaunch {
  const void* q;          // [T, Hq, D] token-major
  const void* k_pool;     // [blocks, Hkv, blk, D]
  const void* v_pool;
  void* o;                // [T, ldo] token-major, ldo >= Hq * D
  const int32_t* bt;      // device: block table [slots, maxb]
  const int32_t* segs;    // device: [nseg, 4] = (row0, n, slot, p0)
  const int32_t* work;    // device: [nwork, 2] = (segment, q-block), heaviest first (pp_fill_work)
  const PpSeg* segs_host; // the host copy of `segs` that the check reads
  int q_bf16, kv_bf16, o_bf16;  // element types of q, of both pools, of o
  int64_t T, Hq, Hkv, D;
  int64_t blocks, blk, slots, maxb;
  int64_t nseg, nwork, ldo;
};

// q-blocks of all segments
inline int64_t pp_work_count(const PpSeg* s, int64_t nseg) {
  int64_t n = 0;
  for (int64_t i = 0; i < nseg; ++i) n += s[i].n > 0 ? ((int64_t)s[i].n + PP_BM - 1) / PP_BM : 0;
  return n;
}

// (segment, q-block) pairs ordered by the number of keys the block streams, most first: the
// workgroups with the longest key loops start first (attn_fwd's heaviest-first order).
inline void pp_fill_work(const PpSeg* s, int64_t nseg, int32_t* work) {
  std::vector<std::pair<int64_t, std::pair<int32_t, int32_t>>> w;
  for (int64_t i = 0; i < nseg; ++i)
    for (int64_t qb = 0; qb * PP_BM < s[i].n; ++qb) {
      const int64_t keys = (int64_t)s[i].p0 + std::min<int64_t>(s[i].n, (qb + 1) * PP_BM);
      w.push_back({-keys, {(int32_t)i, (int32_t)qb}});
    }
  std::stable_sort(w.begin(), w.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  for (size_t i = 0; i < w.size(); ++i) {
    work[2 * i] = w[i].second.first;
    work[2 * i + 1] = w[i].second.second;
  }
}

// Whether the launch is taken (nseg >= 1: the launcher returns 0 for nseg <= 0 before it asks).
inline bool pp_takes(const PpLaunch& L) {
  constexpr int64_t I32 = 0x7fffffff;
  if (!L.q || !L.k_pool || !L.v_pool || !L.o || !L.bt || !L.segs || !L.work || !L.segs_host) return false;
  // dtypes and head_dim: bf16 everywhere, the D = 128 MFMA tiling
  if (!L.q_bf16 || !L.kv_bf16 || !L.o_bf16 || L.D != 128) return false;
  // GQA: whole groups of at most 16 q-heads per KV head (the decode kernels' rule)
  if (L.Hq <= 0 || L.Hkv <= 0 || L.Hq % L.Hkv || L.Hq / L.Hkv > 16) return false;
  // a 64-key tile never straddles a block
  if (L.blk <= 0 || L.blk % 256) return false;
  if (L.T <= 0 || L.blocks <= 0 || L.slots <= 0 || L.maxb <= 0 || L.nseg <= 0) return false;
  // 8-B output stores into rows that hold every head
  if (L.ldo < L.Hq * L.D || L.ldo % 4 || L.ldo > I32) return false;
  // 32-bit offsets of the kernel: byte offsets inside one block (the buffer descriptors' range), key
  // positions of a slot, block-table indices, workgroup ids
  // (as divisions: the products themselves must not overflow 64 bits)
  if (L.blk > I32 / (L.D * 2) || L.maxb > I32 / L.blk || L.slots > I32 / L.maxb) return false;
  if (L.nwork != pp_work_count(L.segs_host, L.nseg) || L.nwork > I32 / L.Hq) return false;
  std::vector<std::pair<int64_t, int64_t>> rows;
  rows.reserve((size_t)L.nseg);
  for (int64_t i = 0; i < L.nseg; ++i) {
    const PpSeg& s = L.segs_host[i];
    const int64_t row0 = s.row0, n = s.n, p0 = s.p0;
    if (n <= 0 || row0 < 0 || row0 + n > L.T) return false;         // rows inside [0, T)
    if (p0 < 0 || p0 + n > L.maxb * L.blk) return false;            // positions the table row can hold
    if (s.slot < 0 || s.slot >= L.slots) return false;              // slot inside the table
    rows.push_back({row0, row0 + n});
  }
  // segments cover disjoint rows of q (two workgroups would store the same output row)
  std::sort(rows.begin(), rows.end());
  for (size_t i = 1; i < rows.size(); ++i)
    if (rows[i].first < rows[i - 1].second) return false;
  return true;
}

}  // namespace mx
