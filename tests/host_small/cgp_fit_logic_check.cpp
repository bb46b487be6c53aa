// csrc/cgp_fit_logic.h on the host: reads cases from the file named on the command line and prints, bit for bit (%a), what the
// header makes of them, for tests/test_cgp_fit_logic_host.py to hold against numpy's arithmetic of cgp._fit_sets.evaluate and
// cgp.rows_from_ww.  Input: the number of cases, then per case  d step | w[P] | lo[P] | hi[P] | val[R]  (P = d + 3,
// R = 1 + 2 P; any strtod spelling, inf and nan included).  Output per case: R lines of 2 d + 2 row entries, one line "f" with
// F_0, one line "g" with P entries.  Stand-alone so that it also runs under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cgp_fit_logic.h"

using namespace ccgp;

static bool read_doubles(FILE* f, std::vector<double>& v) {
  for (double& x : v)
    if (std::fscanf(f, "%lf", &x) != 1) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int cases = 0;
  if (std::fscanf(f, "%d", &cases) != 1 || cases < 0) return 2;
  for (int c = 0; c < cases; ++c) {
    int d = 0;
    double step = 0.0;
    if (std::fscanf(f, "%d %lf", &d, &step) != 2 || d < 1 || d > 61) return 2;
    const int P = cgp_fit_vars(d), R = cgp_fit_rows(d), NC = cgp_fit_cols(d);
    if (P != d + 3 || R != 1 + 2 * P || NC != 2 * d + 2) return 3;
    std::vector<double> w(P), lo(P), hi(P), val(R);
    if (!read_doubles(f, w) || !read_doubles(f, lo) || !read_doubles(f, hi) || !read_doubles(f, val)) return 2;
    for (int r = 0; r < R; ++r) {
      for (int k = 0; k < NC; ++k) std::printf("%a ", cgp_fit_row_entry(w.data(), lo.data(), hi.data(), step, d, r, k));
      std::printf("\n");
    }
    std::printf("f %a\ng", cgp_fit_value(val[0]));
    for (int j = 0; j < P; ++j)
      std::printf(" %a", cgp_fit_grad(val[1 + 2 * j], val[2 + 2 * j], w[j], step, lo[j], hi[j]));
    std::printf("\n");
  }
  std::fclose(f);
  std::printf("ok\n");
  return 0;
}
