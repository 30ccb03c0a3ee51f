// Stand-alone driver of mx::pp_takes, mx::pp_work_count and mx::pp_fill_work
// (csrc/kernels/prefill_paged_args.h), the launch description and the one operand check of the paged-KV
// prefill attention: reads one launch per line from stdin -- `key=value` tokens, integers in any base
// strtoll takes, addresses as integers (never dereferenced), one `seg=row0:n:slot:p0` token per segment,
// missing keys 0 except `nwork` (pp_work_count of the segments) -- and prints per line
// `<pp_takes> <pp_work_count> <segment>:<q-block> ...` (the work table in launch order).
// tests/test_prefill_paged_args.py builds this file plain and under AddressSanitizer + UBSan: the products
// of the overflow rules must not overflow themselves.
#include "kernels/prefill_paged_args.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

using namespace mx;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    PpLaunch L{};
    std::vector<PpSeg> segs;
    bool nwork_given = false;
    std::istringstream ss(line);
    std::string tok;
    while (ss >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) {
        fprintf(stderr, "bad token %s\n", tok.c_str());
        return 2;
      }
      const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
      const long long i = strtoll(v.c_str(), nullptr, 0);
      void* p = reinterpret_cast<void*>((uintptr_t)strtoull(v.c_str(), nullptr, 0));
      if (k == "seg") {
        long long f[4] = {0, 0, 0, 0};
        std::istringstream fs(v);
        std::string part;
        for (int j = 0; j < 4 && std::getline(fs, part, ':'); ++j) f[j] = strtoll(part.c_str(), nullptr, 0);
        segs.push_back({(int32_t)f[0], (int32_t)f[1], (int32_t)f[2], (int32_t)f[3]});
      } else if (k == "q") L.q = p;
      else if (k == "k") L.k_pool = p;
      else if (k == "v") L.v_pool = p;
      else if (k == "o") L.o = p;
      else if (k == "bt") L.bt = (const int32_t*)p;
      else if (k == "segs") L.segs = (const int32_t*)p;
      else if (k == "work") L.work = (const int32_t*)p;
      else if (k == "q_bf16") L.q_bf16 = (int)i;
      else if (k == "kv_bf16") L.kv_bf16 = (int)i;
      else if (k == "o_bf16") L.o_bf16 = (int)i;
      else if (k == "T") L.T = i;
      else if (k == "Hq") L.Hq = i;
      else if (k == "Hkv") L.Hkv = i;
      else if (k == "D") L.D = i;
      else if (k == "blocks") L.blocks = i;
      else if (k == "blk") L.blk = i;
      else if (k == "slots") L.slots = i;
      else if (k == "maxb") L.maxb = i;
      else if (k == "ldo") L.ldo = i;
      else if (k == "nwork") L.nwork = i, nwork_given = true;
      else {
        fprintf(stderr, "unknown key %s\n", k.c_str());
        return 2;
      }
    }
    L.nseg = (int64_t)segs.size();
    L.segs_host = segs.empty() ? nullptr : segs.data();
    const int64_t nw = pp_work_count(segs.data(), L.nseg);
    if (!nwork_given) L.nwork = nw;
    printf("%d %lld", pp_takes(L) ? 1 : 0, (long long)nw);
    if (nw <= 4096) {
      std::vector<int32_t> work((size_t)(2 * nw));
      pp_fill_work(segs.data(), L.nseg, work.data());
      for (int64_t j = 0; j < nw; ++j) printf(" %d:%d", work[2 * j], work[2 * j + 1]);
    }
    printf("\n");
  }
  return 0;
}
