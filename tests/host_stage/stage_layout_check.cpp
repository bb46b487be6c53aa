// csrc/stage_layout.h on the CPU: for each list of pieces, the planning pass (no base) and the carving pass (over a base)
// run the SAME declaration and must end at the same offset; every pointer is 256-byte aligned, and the pieces lie
// inside [base, base + off) without overlapping.  The base is an address that is never dereferenced, so sizes above
// 4 GiB need no memory.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../convex-combination-of-gaussian-processes_amd/csrc/stage_layout.h"

using ccgp::Layout;

struct PieceSpec {
  int elem;        // 1: char, 4: int, 8: double
  size_t count;
};

static void declare(Layout& c, const std::vector<PieceSpec>& ps, std::vector<char*>* out) {
  for (const PieceSpec& p : ps) {
    char* q = p.elem == 8   ? reinterpret_cast<char*>(c.take<double>(p.count))
              : p.elem == 4 ? reinterpret_cast<char*>(c.take<int>(p.count))
                            : c.take<char>(p.count);
    if (out) out->push_back(q);
  }
}

static int check(const char* name, const std::vector<PieceSpec>& ps) {
  std::vector<char*> planned, got;
  Layout plan;
  declare(plan, ps, &planned);
  const size_t bytes = ccgp::layout_bytes([&](Layout& c) { declare(c, ps, nullptr); });
  char* const base = reinterpret_cast<char*>(uintptr_t(1) << 40);
  Layout real(base);
  declare(real, ps, &got);
  int bad = 0;
  if (plan.off != real.off || bytes != real.off) {
    std::printf("%s: planning ends at %zu / %zu, carving at %zu\n", name, plan.off, bytes, real.off);
    ++bad;
  }
  size_t end_prev = 0;
  for (size_t i = 0; i < ps.size(); ++i) {
    const size_t len = ps[i].count * (size_t)ps[i].elem;
    if (planned[i] != nullptr) { std::printf("%s: piece %zu: the planning pass handed out a pointer\n", name, i); ++bad; }
    const size_t off = (size_t)(got[i] - base);
    if (reinterpret_cast<uintptr_t>(got[i]) % 256) { std::printf("%s: piece %zu not 256-byte aligned\n", name, i); ++bad; }
    if (off < end_prev) { std::printf("%s: piece %zu overlaps its predecessor\n", name, i); ++bad; }
    if (off + len > real.off) { std::printf("%s: piece %zu ends at %zu, beyond %zu\n", name, i, off + len, real.off); ++bad; }
    end_prev = off + len;
  }
  return bad;
}

int main() {
  const size_t big = (size_t(5) << 30) / 8 + 3;   // doubles: more than 4 GiB, not a multiple of 256 bytes
  int bad = 0;
  bad += check("empty", {});
  bad += check("one double", {{8, 1}});
  bad += check("loglik_batch n=64 d=4 B=7", {{8, 64 * 4 + 64 + 7 * 10}, {8, 2 * 7 + 4}});
  bad += check("odd int counts", {{8, 33}, {4, 1}, {4, 7}, {8, 5}, {4, 65}, {4, 63}, {8, 1}});
  bad += check("zero-length pieces", {{8, 0}, {8, 12}, {4, 0}, {4, 0}, {8, 32}, {1, 0}});
  bad += check("exact multiples of 256 bytes", {{8, 32}, {4, 64}, {1, 256}, {8, 64}});
  bad += check("bytes then tail", {{1, 1000003}, {8, 17}, {8, 128}});
  bad += check("above 4 GiB", {{8, big}, {4, 3}, {8, big}, {1, (size_t(4) << 30) + 1}, {4, 5}});
  if (bad) return 1;
  std::printf("ok\n");
  return 0;
}
