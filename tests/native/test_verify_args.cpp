// Stand-alone driver of mx::vf_takes (csrc/kernels/verify_args.h), the launch description and the one
// operand check of the verify attention: reads one launch per line from stdin -- `key=value` tokens,
// integers in any base strtoll takes, addresses as integers (never dereferenced), missing keys 0 -- and
// prints `1` or `0` per line.  tests/test_verify_args.py builds this file plain and under
// AddressSanitizer + UBSan: the products of the overflow rules must not overflow themselves.
#include "kernels/verify_args.h"

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
    VfLaunch L{};
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
      if (k == "q") L.q = p;
      else if (k == "k") L.k_pool = p;
      else if (k == "v") L.v_pool = p;
      else if (k == "ks") L.k_scale = (const float*)p;
      else if (k == "vs") L.v_scale = (const float*)p;
      else if (k == "lens") L.lens = (const int32_t*)p;
      else if (k == "nq") L.nq = (const int32_t*)p;
      else if (k == "slots") L.slots = (const int32_t*)p;
      else if (k == "bt") L.bt = (const int32_t*)p;
      else if (k == "ml") L.part_ml = (float*)p;
      else if (k == "po") L.part_o = (float*)p;
      else if (k == "out") L.out = p;
      else if (k == "q_bf16") L.q_bf16 = (int)i;
      else if (k == "out_bf16") L.out_bf16 = (int)i;
      else if (k == "kv_bf16") L.kv_bf16 = (int)i;
      else if (k == "kv_u8") L.kv_u8 = (int)i;
      else if (k == "B") L.B = i;
      else if (k == "n") L.n = i;
      else if (k == "Hq") L.Hq = i;
      else if (k == "Hkv") L.Hkv = i;
      else if (k == "D") L.D = i;
      else if (k == "rows") L.rows = i;
      else if (k == "max_seq") L.max_seq = i;
      else if (k == "maxb") L.maxb = i;
      else if (k == "nsplit") L.nsplit = i;
      else {
        fprintf(stderr, "unknown key %s\n", k.c_str());
        return 2;
      }
    }
    printf("%d\n", vf_takes(L) ? 1 : 0);
  }
  return 0;
}
