// wg_allowed.h -- flat image of the AllowedIPs table and the walker both sides run.
//
// NepTUN keeps two relations: the route
// network -> peer (Device::peers_by_ip, device/mod.rs:533-564, walked by
// AllowedIps::find, allowed_ips.rs:49, for every outbound packet) and the ownership
// peer -> its networks (Peer::allowed_ips, peer.rs:178, asked for every decrypted
// packet's source).  wg_allowed.cpp holds both on the host and flattens them into one
// image of 8-byte words that is mirrored into HBM (wg_gpu_allowed_set); the functions
// below walk that image and are compiled for the host and for the device.
//
// Image (every index is stored + 1, 0 = none):
//   slots   per family a multibit trie with an 8-bit stride: node k is the 256 slots
//           slots[256 k ..]; slot = {child node, head}.  A network of prefix length
//           8 d + r (r in 1..8) sits in its depth-d node, expanded over its 2^(8-r)
//           slots; the builder inserts in order of rising length, so inside a node a
//           longer prefix overwrites a shorter one.  Length 0 is the family's def[].
//   heads   one per stored network: {route value of the longest routed network at or
//           above it, or WG_ALLOWED_NONE; first owner record}.
//   owners  {value, next}: a network's owners, running on into the owners of the next
//           shorter stored network that covers it -- every owner of every network
//           that contains an address is on the chain its longest match starts.
// A lookup keeps the last non-zero head on its way down: at most 4 dependent slot
// loads (IPv4) or 16 (IPv6), one head load, and for contains the owner chain.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <memory>
#include <vector>

#include "neptun_gpu.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WG_ALLOWED_HD __host__ __device__
#else
#define WG_ALLOWED_HD
#endif

#ifndef WG_ALLOWED_NONE
#define WG_ALLOWED_NONE 0xFFFFFFFFu
#endif

namespace wg {

struct alignas(8) AllowedWord {
  uint32_t x, y;
};

struct AllowedView {
  const AllowedWord *slots = nullptr;
  const AllowedWord *heads = nullptr;
  const AllowedWord *owners = nullptr;
  uint32_t root[2] = {0, 0};  // [0] IPv4, [1] IPv6: root node + 1
  uint32_t def[2] = {0, 0};   // head + 1 of the family's /0
  uint32_t n_nodes = 0, n_heads = 0, n_owners = 0;
};

// An address as big-endian words: IPv4 in w[0], IPv6 in w[0..3].
struct AllowedAddr {
  uint32_t w[4];
};

WG_ALLOWED_HD inline uint32_t allowed_be32(const uint8_t *p) {
  return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3];
}

// head + 1 of the longest stored network containing `a` (0: none)
// (four strides down from `node` along the bytes of w; false: the path ended)
WG_ALLOWED_HD inline bool allowed_walk_word(const AllowedView &v, uint32_t w, uint32_t &node, uint32_t &best) {
#pragma unroll
  for (uint32_t sh = 32; sh != 0;) {
    sh -= 8;
    if (node == 0 || node > v.n_nodes) return false;
    const AllowedWord s = v.slots[(uint64_t)(node - 1u) * 256u + ((w >> sh) & 0xFFu)];
    if (s.y) best = s.y;
    node = s.x;
  }
  return true;
}

WG_ALLOWED_HD inline uint32_t allowed_walk(const AllowedView &v, uint32_t v6, const AllowedAddr &a) {
  uint32_t best = v6 ? v.def[1] : v.def[0], node = v6 ? v.root[1] : v.root[0];
  // (spelled out word by word: the address stays in registers on the device)
  if (!allowed_walk_word(v, a.w[0], node, best) || !v6) return best;
  if (!allowed_walk_word(v, a.w[1], node, best)) return best;
  if (!allowed_walk_word(v, a.w[2], node, best)) return best;
  allowed_walk_word(v, a.w[3], node, best);
  return best;
}

// AllowedIps::find: the route value of the longest routed network containing `a`
WG_ALLOWED_HD inline uint32_t allowed_find(const AllowedView &v, uint32_t v6, const AllowedAddr &a) {
  const uint32_t h = allowed_walk(v, v6, a);
  if (h == 0 || h > v.n_heads) return WG_ALLOWED_NONE;
  return v.heads[h - 1u].x;
}

// Peer::is_allowed_ip: does any network owned by `value` contain `a`
WG_ALLOWED_HD inline bool allowed_contains(const AllowedView &v, uint32_t v6, const AllowedAddr &a,
                                           uint32_t value) {
  const uint32_t h = allowed_walk(v, v6, a);
  if (h == 0 || h > v.n_heads) return false;
  uint32_t o = v.heads[h - 1u].y;
  for (uint32_t steps = 0; o != 0 && o <= v.n_owners && steps < v.n_owners; ++steps) {
    const AllowedWord r = v.owners[o - 1u];
    if (r.x == value) return true;
    o = r.y;
  }
  return false;
}

// Tunn::dst_address (noise/mod.rs:205-223) / the source address
// validate_decapsulated_packet reads (mod.rs:606-659) of a host packet:
// 0 = none, else 4 or 6 with the address in `a`.
inline uint32_t allowed_packet_addr(const uint8_t *p, uint32_t len, bool source, AllowedAddr &a) {
  if (len < 20) return 0;
  const uint32_t ver = p[0] >> 4;
  if (ver == 4) {
    a.w[0] = allowed_be32(p + (source ? 12 : 16));
    a.w[1] = a.w[2] = a.w[3] = 0;
    return 4;
  }
  if (ver == 6 && len >= 40) {
    const uint8_t *q = p + (source ? 8 : 24);
    for (int k = 0; k < 4; ++k) a.w[k] = allowed_be32(q + 4 * k);
    return 6;
  }
  return 0;
}

#if defined(__HIPCC__)
// wg_allowed.hip
__global__ void allowed_route_kernel(wg_packet_desc *descs, uint32_t n, const uint8_t *src,
                                     AllowedView v, uint32_t *value_out, uint32_t set_key_slot);
__global__ void allowed_filter_kernel(const wg_packet_desc *descs, uint32_t n, const uint8_t *dst,
                                      const int32_t *status, const uint32_t *expect,
                                      uint32_t slot_shift, AllowedView v, uint8_t *allowed_out);
#endif

}  // namespace wg

// wg_allowed.cpp, for wg_gpu.cpp and wg_tunn.cpp: the table's current image (rebuilt
// if the table changed since the last one).  The view points into the returned
// object, which stays valid for as long as the caller holds it.
struct wg_allowed;
namespace wg {
struct AllowedImage {
  std::vector<AllowedWord> words;  // slots | heads | owners
  AllowedView view;                // host pointers into `words`
  size_t heads_at = 0, owners_at = 0;
};
std::shared_ptr<const AllowedImage> allowed_image(wg_allowed *a);
}  // namespace wg
