// allowed_check.cpp -- the AllowedIPs host table and walker on their own, for a CPU
// sanitizer run (no GPU, no Python):
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ineptun_amd/csrc tools/probes/allowed_check.cpp neptun_amd/csrc/wg_allowed.cpp \
//       -o build/allowed_check && build/allowed_check
// Random inserts / removals / collisions / a clear, and after every stage every lookup
// against a brute-force scan of the two relations (as tests/allowed_model.py does).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <map>
#include <array>
#include <vector>

#include "neptun_gpu.h"

static const char *g_err = "";
int wg_fail_msg(int rc, const char *what) {  // (wg_gpu.cpp's, for the stand-alone build)
  g_err = what;
  return rc;
}

namespace {
using Addr = std::array<uint8_t, 16>;
struct Net {
  int fam;
  Addr a;
  uint32_t cidr;
  bool operator<(const Net &o) const {
    if (fam != o.fam) return fam < o.fam;
    if (cidr != o.cidr) return cidr < o.cidr;
    return a < o.a;
  }
};
Addr truncate(const Addr &a, int fam, uint32_t cidr) {
  Addr r{};
  const uint32_t bytes = fam == 4 ? 4 : 16;
  for (uint32_t k = 0; k < bytes; ++k) {
    const uint32_t keep = cidr >= 8 * (k + 1) ? 8 : cidr > 8 * k ? cidr - 8 * k : 0;
    r[k] = (uint8_t)(a[k] & (0xFF00u >> keep));
  }
  return r;
}
bool covers(const Net &n, int fam, const Addr &a) { return n.fam == fam && truncate(a, fam, n.cidr) == n.a; }

struct Model {
  std::map<Net, uint32_t> route;
  std::set<std::pair<Net, uint32_t>> owned;
  uint32_t find(int fam, const Addr &a) const {
    uint32_t best = WG_ALLOWED_NONE;
    int len = -1;
    for (const auto &r : route)
      if (covers(r.first, fam, a) && (int)r.first.cidr > len) {
        len = (int)r.first.cidr;
        best = r.second;
      }
    return best;
  }
  bool contains(int fam, const Addr &a, uint32_t v) const {
    for (const auto &o : owned)
      if (o.second == v && covers(o.first, fam, a)) return true;
    return false;
  }
};

int compare(wg_allowed *t, const Model &m, std::mt19937_64 &rng, const std::vector<Net> &nets, int probes) {
  int bad = 0;
  for (int p = 0; p < probes; ++p) {
    Addr a;
    for (auto &b : a) b = (uint8_t)rng();
    int fam = rng() % 5 < 3 ? 4 : 6;
    if (!nets.empty() && rng() % 5 < 3) {  // under a stored network
      const Net &n = nets[rng() % nets.size()];
      fam = n.fam;
      const Addr top = truncate(a, fam, n.cidr);
      for (int k = 0; k < 16; ++k) a[k] = (uint8_t)(n.a[k] | (a[k] ^ top[k]));
    }
    uint32_t v = 0;
    if (wg_allowed_find(t, fam, a.data(), &v) != 0 || v != m.find(fam, a)) ++bad;
    for (uint32_t val = 0; val < 48; ++val)
      if (wg_allowed_contains(t, fam, a.data(), val) != (m.contains(fam, a, val) ? 1 : 0)) ++bad;
  }
  return bad;
}
}  // namespace

int main() {
  int bad = 0;
  static const uint32_t l4[] = {0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32};
  static const uint32_t l6[] = {0, 1, 7, 8, 9, 63, 64, 65, 120, 127, 128};
  for (uint64_t seed = 1; seed <= 3; ++seed) {
    std::mt19937_64 rng(seed);
    wg_allowed *t = nullptr;
    if (wg_allowed_create(&t) != 0) return 2;
    Model m;
    std::vector<Net> nets;
    bad += compare(t, m, rng, nets, 50);  // the empty table
    for (int k = 0; k < 160; ++k) {
      Net n;
      n.fam = rng() % 5 < 3 ? 4 : 6;
      n.cidr = n.fam == 4 ? l4[rng() % 13] : l6[rng() % 11];
      Addr a;
      for (auto &b : a) b = (uint8_t)rng();
      if (k >= 40 && rng() % 2) {  // nested under a stored network of the family
        const Net &p = nets[rng() % nets.size()];
        if (p.fam == n.fam && p.cidr < n.cidr) {
          const Addr top = truncate(a, n.fam, p.cidr);
          for (int j = 0; j < 16; ++j) a[j] = (uint8_t)(p.a[j] | (a[j] ^ top[j]));
        }
      }
      const uint32_t value = (uint32_t)(rng() % 48);
      if (wg_allowed_insert(t, n.fam, a.data(), n.cidr, value) != 0) return 3;
      n.a = truncate(a, n.fam, n.cidr);
      m.route[n] = value;
      m.owned.emplace(n, value);
      nets.push_back(n);
      if (k % 31 == 30) {  // a collision
        const Net &c = nets[rng() % nets.size()];
        const uint32_t v2 = (uint32_t)(rng() % 48);
        wg_allowed_insert(t, c.fam, c.a.data(), c.cidr, v2);
        m.route[c] = v2;
        m.owned.emplace(c, v2);
      }
      if (k % 23 == 22) {
        const uint32_t gone = (uint32_t)(rng() % 48);
        wg_allowed_remove_value(t, gone);
        for (auto it = m.owned.begin(); it != m.owned.end();) it = it->second == gone ? m.owned.erase(it) : std::next(it);
        for (auto it = m.route.begin(); it != m.route.end();) it = it->second == gone ? m.route.erase(it) : std::next(it);
      }
      if (k % 40 == 39) bad += compare(t, m, rng, nets, 300);
      if (wg_allowed_count(t) != m.route.size()) ++bad;
    }
    bad += compare(t, m, rng, nets, 2000);
    uint8_t z[16] = {0};
    if (wg_allowed_insert(t, 4, z, 33, 1) != WG_RC_INVALID_ARGUMENT) ++bad;
    if (wg_allowed_insert(t, 6, z, 129, 1) != WG_RC_INVALID_ARGUMENT) ++bad;
    wg_allowed_clear(t);
    m = Model{};
    bad += compare(t, m, rng, nets, 200);
    wg_allowed_destroy(t);
  }
  std::printf("allowed_check: %d mismatches\n", bad);
  return bad ? 1 : 0;
}
