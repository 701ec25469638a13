// wg_allowed.cpp -- the AllowedIPs table on the host (include/neptun_gpu.h wg_allowed_*).
//
// Two relations, as the reference keeps them (they can disagree):
//   route   network -> value, the last insert of a network wins (Device::peers_by_ip;
//           device/mod.rs:533-534 and :564 drop a peer's routes by their current value);
//   owned   (network, value) pairs (each Peer's own allowed_ips, peer.rs:178).
// Lookups go through the flat image of wg_allowed.h, rebuilt lazily after a change:
// the host answers with the very words and the very walker the device uses.
// Plain C++: nothing here needs a GPU.
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <set>
#include <utility>
#include <vector>

#include "neptun_gpu.h"
#include "wg_allowed.h"

int wg_fail_msg(int rc, const char *what);  // wg_gpu.cpp: sets wg_gpu_last_error

namespace {

// (cidr first: std::map / std::set walk the networks in order of rising prefix length)
struct Net {
  uint8_t v6 = 0, cidr = 0;
  uint8_t addr[16] = {0};
  bool operator<(const Net &o) const {
    if (v6 != o.v6) return v6 < o.v6;
    if (cidr != o.cidr) return cidr < o.cidr;
    return std::memcmp(addr, o.addr, 16) < 0;
  }
  bool operator==(const Net &o) const { return v6 == o.v6 && cidr == o.cidr && !std::memcmp(addr, o.addr, 16); }
};

wg::AllowedAddr words_of(const uint8_t addr[16], bool v6) {
  wg::AllowedAddr a;
  for (int k = 0; k < 4; ++k) a.w[k] = (v6 || k == 0) ? wg::allowed_be32(addr + 4 * k) : 0u;
  return a;
}

}  // namespace

struct wg_allowed {
  std::mutex mu;
  std::map<Net, uint32_t> route;
  std::set<std::pair<Net, uint32_t>> owned;
  std::shared_ptr<const wg::AllowedImage> image;  // null: stale
};

namespace {

// The image of (route, owned): see wg_allowed.h.  Networks are added in order of rising
// prefix length, so when one is added every shorter network that covers it is final:
// a walk of the half-built image finds the longest of them, whose route the new head
// inherits and whose owner chain the new network's owners run on into.
std::shared_ptr<const wg::AllowedImage> build_image(const wg_allowed &t) {
  using wg::AllowedWord;
  struct Entry {
    bool routed = false;
    uint32_t value = WG_ALLOWED_NONE;
    std::vector<uint32_t> owners;
  };
  std::map<Net, Entry> nets;
  for (const auto &r : t.route) {
    Entry &e = nets[r.first];
    e.routed = true;
    e.value = r.second;
  }
  for (const auto &o : t.owned) nets[o.first].owners.push_back(o.second);

  std::vector<AllowedWord> slots, heads, owners;
  wg::AllowedView v;  // over the vectors above, refreshed before every walk
  auto new_node = [&]() -> uint32_t {
    slots.resize(slots.size() + 256, AllowedWord{0, 0});
    return (uint32_t)(slots.size() / 256);  // index + 1
  };
  for (const auto &kv : nets) {
    const Net &n = kv.first;
    const Entry &e = kv.second;
    if (slots.size() / 256 + 17 > (1u << 21)) return nullptr;  // 4 GiB of slots: refuse
    if (!v.root[n.v6]) v.root[n.v6] = new_node();
    v.slots = slots.data();
    v.heads = heads.data();
    v.owners = owners.data();
    v.n_nodes = (uint32_t)(slots.size() / 256);
    v.n_heads = (uint32_t)heads.size();
    v.n_owners = (uint32_t)owners.size();
    const uint32_t parent = wg::allowed_walk(v, n.v6, words_of(n.addr, n.v6));
    AllowedWord head{WG_ALLOWED_NONE, 0};
    if (parent) head = heads[parent - 1];
    if (e.routed) head.x = e.value;
    for (size_t k = e.owners.size(); k-- > 0;) {  // (pushed in reverse: the chain reads in set order)
      owners.push_back(AllowedWord{e.owners[k], head.y});
      head.y = (uint32_t)owners.size();
    }
    heads.push_back(head);
    const uint32_t h = (uint32_t)heads.size();
    if (n.cidr == 0) {
      v.def[n.v6] = h;
      continue;
    }
    const uint32_t depth = (n.cidr - 1u) / 8u, r = n.cidr - 8u * depth;  // r in 1..8
    uint32_t node = v.root[n.v6];
    for (uint32_t d = 0; d < depth; ++d) {
      const size_t at = (size_t)(node - 1) * 256 + n.addr[d];
      if (!slots[at].x) {
        const uint32_t c = new_node();  // (may move `slots`)
        slots[at].x = c;
      }
      node = slots[at].x;
    }
    const uint32_t first = n.addr[depth], count = 1u << (8u - r);
    for (uint32_t s = first; s < first + count; ++s) slots[(size_t)(node - 1) * 256 + s].y = h;
  }

  auto img = std::make_shared<wg::AllowedImage>();
  img->heads_at = slots.size();
  img->owners_at = slots.size() + heads.size();
  img->words.reserve(slots.size() + heads.size() + owners.size());
  img->words.insert(img->words.end(), slots.begin(), slots.end());
  img->words.insert(img->words.end(), heads.begin(), heads.end());
  img->words.insert(img->words.end(), owners.begin(), owners.end());
  v.slots = img->words.data();
  v.heads = img->words.data() + img->heads_at;
  v.owners = img->words.data() + img->owners_at;
  v.n_nodes = (uint32_t)(slots.size() / 256);
  v.n_heads = (uint32_t)heads.size();
  v.n_owners = (uint32_t)owners.size();
  img->view = v;
  return img;
}

}  // namespace

namespace wg {
std::shared_ptr<const AllowedImage> allowed_image(wg_allowed *a) {
  std::lock_guard<std::mutex> lk(a->mu);
  if (!a->image) a->image = build_image(*a);
  return a->image;
}
}  // namespace wg

extern "C" {

int wg_allowed_create(wg_allowed **out) {
  if (!out) return wg_fail_msg(WG_RC_INVALID_ARGUMENT, "allowed_create: null argument");
  *out = new (std::nothrow) wg_allowed;
  if (!*out) return wg_fail_msg(WG_RC_OUT_OF_MEMORY, "allowed_create: host alloc");
  return WG_RC_OK;
}

int wg_allowed_destroy(wg_allowed *a) {
  delete a;
  return WG_RC_OK;
}

int wg_allowed_insert(wg_allowed *a, int family, const uint8_t addr[16], uint32_t cidr, uint32_t value) {
  if (!a || !addr) return wg_fail_msg(WG_RC_INVALID_ARGUMENT, "allowed_insert: null argument");
  if (family != 4 && family != 6) return wg_fail_msg(WG_RC_INVALID_ARGUMENT, "allowed_insert: family is 4 or 6");
  const uint32_t bits = family == 4 ? 32u : 128u;
  if (cidr > bits) return wg_fail_msg(WG_RC_INVALID_ARGUMENT, "allowed_insert: prefix longer than the address");
  if (value == WG_ALLOWED_NONE)
    return wg_fail_msg(WG_RC_INVALID_ARGUMENT, "allowed_insert: value 0xFFFFFFFF is WG_ALLOWED_NONE");
  Net n;
  n.v6 = family == 6;
  n.cidr = (uint8_t)cidr;
  for (uint32_t k = 0; k < bits / 8u; ++k) {  // IpNetwork::new_truncate: host bits cleared
    const uint32_t keep = cidr >= 8u * (k + 1u) ? 8u : cidr > 8u * k ? cidr - 8u * k : 0u;
    n.addr[k] = (uint8_t)(addr[k] & (0xFF00u >> keep));
  }
  std::lock_guard<std::mutex> lk(a->mu);
  a->route[n] = value;
  a->owned.emplace(n, value);
  a->image.reset();
  return WG_RC_OK;
}

int wg_allowed_remove_value(wg_allowed *a, uint32_t value) {
  if (!a) return wg_fail_msg(WG_RC_INVALID_ARGUMENT, "allowed_remove_value: null argument");
  std::lock_guard<std::mutex> lk(a->mu);
  for (auto it = a->owned.begin(); it != a->owned.end();) it = it->second == value ? a->owned.erase(it) : std::next(it);
  for (auto it = a->route.begin(); it != a->route.end();) it = it->second == value ? a->route.erase(it) : std::next(it);
  a->image.reset();
  return WG_RC_OK;
}

int wg_allowed_clear(wg_allowed *a) {
  if (!a) return wg_fail_msg(WG_RC_INVALID_ARGUMENT, "allowed_clear: null argument");
  std::lock_guard<std::mutex> lk(a->mu);
  a->route.clear();
  a->owned.clear();
  a->image.reset();
  return WG_RC_OK;
}

uint32_t wg_allowed_count(const wg_allowed *a) {
  if (!a) return 0;
  wg_allowed *m = const_cast<wg_allowed *>(a);
  std::lock_guard<std::mutex> lk(m->mu);
  return (uint32_t)m->route.size();
}

int wg_allowed_find(wg_allowed *a, int family, const uint8_t addr[16], uint32_t *value) {
  if (!a || !addr || !value) return wg_fail_msg(WG_RC_INVALID_ARGUMENT, "allowed_find: null argument");
  if (family != 4 && family != 6) return wg_fail_msg(WG_RC_INVALID_ARGUMENT, "allowed_find: family is 4 or 6");
  const auto img = wg::allowed_image(a);
  if (!img) return wg_fail_msg(WG_RC_OUT_OF_MEMORY, "allowed_find: the table's image is too large");
  *value = wg::allowed_find(img->view, family == 6, words_of(addr, family == 6));
  return WG_RC_OK;
}

int wg_allowed_contains(wg_allowed *a, int family, const uint8_t addr[16], uint32_t value) {
  if (!a || !addr) return wg_fail_msg(WG_RC_INVALID_ARGUMENT, "allowed_contains: null argument");
  if (family != 4 && family != 6) return wg_fail_msg(WG_RC_INVALID_ARGUMENT, "allowed_contains: family is 4 or 6");
  const auto img = wg::allowed_image(a);
  if (!img) return wg_fail_msg(WG_RC_OUT_OF_MEMORY, "allowed_contains: the table's image is too large");
  return wg::allowed_contains(img->view, family == 6, words_of(addr, family == 6), value) ? 1 : 0;
}

}  // extern "C"
