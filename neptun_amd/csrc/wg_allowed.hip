// wg_allowed.hip -- AllowedIPs on the device: outbound routing and inbound source filter.
//
// NepTUN routes every outbound packet by longest-prefix match of its destination
// address (device/mod.rs:1295-1313: Tunn::dst_address, noise/mod.rs:205-223, then
// AllowedIps::find, allowed_ips.rs:49) and writes a decrypted packet to the TUN only
// if its source address lies in one of the sending peer's networks
// (peer.is_allowed_ip, device/mod.rs:1056, peer.rs:178).  Both run here one lane per
// descriptor over the flat table image of wg_allowed.h (the walker is the host's).
// No LDS, no atomics: per packet the 32-byte descriptor, one line of the IP header,
// at most 4 (IPv4) or 16 (IPv6) dependent 8-byte slot loads that an L2-resident table
// serves, one head load (filter: plus the owner chain), and the route's two dword
// stores or the filter's one byte.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "neptun_gpu.h"
#include "wg_allowed.h"

namespace wg {

namespace {

// The header fields as the reference reads them, from a packet of `len` bytes at h:
// the version nibble, then 4 address bytes at `o4` (version 4, len >= 20) or 16 at
// `o6` (version 6, len >= 40).  Returns 0 (no address), 4 or 6.  Dword loads when h
// is 4-aligned (o4 and o6 are multiples of 4), bytewise otherwise; nothing outside
// [h, h + len) is read.
__device__ inline uint32_t header_addr(const uint8_t *h, uint32_t len, uint32_t o4, uint32_t o6,
                                       AllowedAddr &out) {
  uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0, fam = 0;  // (scalars: a struct filled on some paths went to scratch)
  if (len < 20u) return 0;
  const bool aligned = (reinterpret_cast<uintptr_t>(h) & 3u) == 0;
  const uint32_t ver = (aligned ? (reinterpret_cast<const uint32_t *>(h)[0] & 0xFFu) : (uint32_t)h[0]) >> 4;
  if (ver == 4u) {
    w0 = aligned ? __builtin_bswap32(reinterpret_cast<const uint32_t *>(h + o4)[0]) : allowed_be32(h + o4);
    fam = 4;
  } else if (ver == 6u && len >= 40u) {
    if (aligned) {
      const uint32_t *q = reinterpret_cast<const uint32_t *>(h + o6);
      w0 = __builtin_bswap32(q[0]);
      w1 = __builtin_bswap32(q[1]);
      w2 = __builtin_bswap32(q[2]);
      w3 = __builtin_bswap32(q[3]);
    } else {
      w0 = allowed_be32(h + o6);
      w1 = allowed_be32(h + o6 + 4);
      w2 = allowed_be32(h + o6 + 8);
      w3 = allowed_be32(h + o6 + 12);
    }
    fam = 6;
  }
  out = AllowedAddr{{w0, w1, w2, w3}};
  return fam;
}

}  // namespace

__global__ __launch_bounds__(256) void allowed_route_kernel(wg_packet_desc *descs, uint32_t n,
                                                            const uint8_t *src, AllowedView v,
                                                            uint32_t *value_out, uint32_t set_key_slot) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint64_t off = descs[i].src_off;
  const uint32_t len = descs[i].len;
  uint32_t value = WG_ALLOWED_NONE;
  AllowedAddr a;
  const uint32_t fam = header_addr(src + off, len, 16u, 24u, a);  // dst_address: bytes 16..20 / 24..40
  if (fam) value = allowed_find(v, fam == 6u, a);
  if (value_out) value_out[i] = value;
  if (set_key_slot) descs[i].key_slot = value;
}

__global__ __launch_bounds__(256) void allowed_filter_kernel(const wg_packet_desc *descs, uint32_t n,
                                                             const uint8_t *dst, const int32_t *status,
                                                             const uint32_t *expect, uint32_t slot_shift,
                                                             AllowedView v, uint8_t *allowed_out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint64_t off = descs[i].dst_off;
  const uint32_t len = descs[i].len;
  const uint32_t e = expect ? expect[i] : descs[i].key_slot >> slot_shift;
  uint8_t ok = 0;
  if (status[i] == WG_STATUS_OK && len > WG_DATA_OVERHEAD_SZ) {  // (a keepalive has no source)
    AllowedAddr a;
    // the source address: bytes 12..16 / 8..24 of the plaintext (len - 32 bytes)
    const uint32_t fam = header_addr(dst + off, len - WG_DATA_OVERHEAD_SZ, 12u, 8u, a);
    if (fam) ok = allowed_contains(v, fam == 6u, a, e) ? 1 : 0;
  }
  allowed_out[i] = ok;
}

}  // namespace wg
