// Prints, for every n 1..128 at a few (d, K, m), what csrc/small_layout.h says about the kept-factor prediction:
//   n d K m small_reg_sites_supported small_reg_sites_scratch
// tests/test_failure_contract_host.py holds the Python mirrors of tests/test_gpu_failure_contract.py to these lines.
#include <cstdio>

#include "small_layout.h"

int main() {
  const int ds[] = {1, 5, 9, 63}, Ks[] = {1, 2, 3, 4}, ms[] = {1, 65, 129};
  for (int n = 1; n <= 128; ++n)
    for (int d : ds)
      for (int K : Ks)
        for (int m : ms)
          std::printf("%d %d %d %d %d %zu\n", n, d, K, m, ccgp::small_reg_sites_supported(n, d, K) ? 1 : 0,
                      ccgp::small_reg_sites_scratch(n, d, K, m));
  return 0;
}
