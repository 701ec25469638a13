"""AllowedIPs table (include/neptun_gpu.h wg_allowed_*) -- Python face.

The host side of the device routing: the route (network -> value, last insert
wins) and the ownership (value -> its networks) of NepTUN's Device::peers_by_ip
and Peer::allowed_ips.  Needs no GPU; `GpuContext.allowed_set` mirrors it into HBM.
"""
from __future__ import annotations

import ctypes
import ipaddress

from ._native import check, load

NONE = 0xFFFFFFFF  # WG_ALLOWED_NONE


def _addr(addr, family=None):
    """(family, 16-byte buffer) of a str, bytes (4 or 16) or ipaddress address."""
    if isinstance(addr, str):
        addr = ipaddress.ip_address(addr)
    if isinstance(addr, (ipaddress.IPv4Address, ipaddress.IPv6Address)):
        raw = addr.packed
    else:
        raw = bytes(addr)
    if len(raw) not in (4, 16):
        raise ValueError("an address is 4 or 16 bytes")
    fam = 4 if len(raw) == 4 else 6
    if family is not None and family != fam:
        raise ValueError("address family mismatch")
    return fam, ctypes.create_string_buffer(raw.ljust(16, b"\0"), 16)


class AllowedIps:
    """wg_allowed: insert / remove_value / clear / find / contains / len()."""

    def __init__(self, lib_path: str | None = None):
        self._lib = load(lib_path) if lib_path else load()
        h = ctypes.c_void_p()
        check(self._lib.wg_allowed_create(ctypes.byref(h)), "wg_allowed_create", self._lib)
        self._h = h

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._lib.wg_allowed_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def insert(self, addr, cidr: int | None = None, value: int = 0) -> None:
        """insert("10.0.0.0/8", value=3), insert("10.0.0.0", 8, 3), insert(ip_network, value=3),
        insert(b"\\x0a\\0\\0\\0", 8, 3).  Host bits are cleared; the network's route becomes
        `value` and `value` owns the network."""
        if isinstance(addr, str) and "/" in addr:
            addr = ipaddress.ip_network(addr, strict=False)
        if isinstance(addr, (ipaddress.IPv4Network, ipaddress.IPv6Network)):
            if cidr is None:
                cidr = addr.prefixlen
            addr = addr.network_address
        if cidr is None:
            raise ValueError("insert needs a prefix length")
        fam, buf = _addr(addr)
        check(self._lib.wg_allowed_insert(self._h, fam, buf, int(cidr), int(value)), "wg_allowed_insert",
              self._lib)

    def remove_value(self, value: int) -> None:
        check(self._lib.wg_allowed_remove_value(self._h, int(value)), "wg_allowed_remove_value", self._lib)

    def clear(self) -> None:
        check(self._lib.wg_allowed_clear(self._h), "wg_allowed_clear", self._lib)

    def __len__(self) -> int:
        return int(self._lib.wg_allowed_count(self._h))

    def find(self, addr):
        """The route value of the longest routed network containing addr, or None."""
        fam, buf = _addr(addr)
        v = ctypes.c_uint32()
        check(self._lib.wg_allowed_find(self._h, fam, buf, ctypes.byref(v)), "wg_allowed_find", self._lib)
        return None if v.value == NONE else v.value

    def contains(self, addr, value: int) -> bool:
        """Does any network owned by `value` contain addr."""
        fam, buf = _addr(addr)
        rc = self._lib.wg_allowed_contains(self._h, fam, buf, int(value))
        if rc < 0:
            check(rc, "wg_allowed_contains", self._lib)
        return bool(rc)


__all__ = ["AllowedIps", "NONE"]
