"""The AllowedIPs host table (neptun_amd/csrc/wg_allowed.cpp, through ctypes) against
the brute-force model of tests/allowed_model.py.  No GPU: the table's lookups walk the
flat image the device gets, with the walker the kernels use (wg_allowed.h).

Semantics restated from the reference: the route is Device::peers_by_ip (last insert
of a network wins, device/mod.rs:533-564), the ownership each Peer's allowed_ips
(peer.rs:178); insert truncates host bits (allowed_ips.rs:45).
"""
import ctypes
import ipaddress

import pytest

import neptun_amd
from neptun_amd import AllowedIps

import allowed_model as AM

A, B, C, D = 1, 2, 3, 4


def test_host_bits_are_truncated():
    t = AllowedIps()
    t.insert("10.1.2.3", 16, A)
    assert len(t) == 1
    assert t.find("10.1.0.0") == A and t.find("10.1.255.255") == A
    assert t.find("10.2.2.3") is None
    t.insert("10.1.99.99/16", value=B)  # the same network: one entry, B's route
    assert len(t) == 1 and t.find("10.1.2.3") == B
    t.insert("2001:db8:ffff::1", 32, C)
    assert t.find("2001:db8::") == C and t.find("2001:db9::") is None
    t.insert(bytes([192, 168, 7, 255]), 25, D)
    assert t.find("192.168.7.128") == D and t.find("192.168.7.127") is None


@pytest.mark.parametrize("cidr", [0, 1, 8, 9, 31, 32])
def test_v4_prefix_lengths(cidr):
    t, m = AllowedIps(), AM.Model()
    base = int(ipaddress.IPv4Address("173.201.94.77"))
    for x in (t_ := AM.Adapter(t), m):
        x.insert(4, base, cidr, A)
    net = base & AM.mask(4, cidr)
    span = 1 << (32 - cidr)
    probes = {net, net + span - 1, (net - 1) % 2**32, (net + span) % 2**32, base, base ^ 1,
              base ^ (1 << 31), 0, 2**32 - 1}
    if cidr < 32:
        probes.add(net + span // 2)
    for a in probes:
        assert t_.find(4, a) == m.find(4, a), (cidr, a)
        assert t_.contains(4, a, A) == m.contains(4, a, A), (cidr, a)
    assert t_.find(4, net) == A and t.find("::") is None


@pytest.mark.parametrize("cidr", [0, 1, 63, 64, 65, 127, 128])
def test_v6_prefix_lengths(cidr):
    t, m = AllowedIps(), AM.Model()
    base = int(ipaddress.IPv6Address("2a03:2880:f12f:83:face:b00c:0:25de"))
    for x in (t_ := AM.Adapter(t), m):
        x.insert(6, base, cidr, A)
    net = base & AM.mask(6, cidr)
    span = 1 << (128 - cidr)
    probes = {net, net + span - 1, (net - 1) % 2**128, (net + span) % 2**128, base, base ^ 1,
              base ^ (1 << 127), base ^ (1 << 64), base ^ (1 << 63), 0, 2**128 - 1}
    for a in probes:
        assert t_.find(6, a) == m.find(6, a), (cidr, a)
        assert t_.contains(6, a, A) == m.contains(6, a, A), (cidr, a)
    assert t_.find(6, net) == A and t.find("0.0.0.0") is None


def test_too_long_prefixes_are_refused():
    t = AllowedIps()
    with pytest.raises(neptun_amd.NeptunGpuError, match="prefix longer"):
        t.insert("10.0.0.0", 33, A)
    with pytest.raises(neptun_amd.NeptunGpuError, match="prefix longer"):
        t.insert("fd00::", 129, A)
    with pytest.raises(neptun_amd.NeptunGpuError, match="WG_ALLOWED_NONE"):
        t.insert("10.0.0.0", 8, 0xFFFFFFFF)
    assert len(t) == 0 and t.find("10.0.0.1") is None


def test_nested_prefixes_with_different_values():
    t = AllowedIps()
    t.insert("10.0.0.0/8", value=A)
    t.insert("10.20.0.0/16", value=B)
    t.insert("10.20.30.0/24", value=C)
    t.insert("10.20.30.40/32", value=D)
    assert t.find("10.20.30.40") == D
    assert t.find("10.20.30.41") == C
    assert t.find("10.20.31.40") == B
    assert t.find("10.21.30.40") == A
    assert t.find("11.20.30.40") is None
    for v in (A, B, C, D):
        assert t.contains("10.20.30.40", v)
    assert [t.contains("10.20.30.41", v) for v in (A, B, C, D)] == [True, True, True, False]
    assert [t.contains("10.21.0.0", v) for v in (A, B, C, D)] == [True, False, False, False]
    assert len(t) == 4


def test_default_routes_of_the_two_families_are_independent():
    t = AllowedIps()
    t.insert("0.0.0.0/0", value=A)
    assert t.find("203.0.113.9") == A and t.find("2001:db8::1") is None
    assert t.contains("8.8.8.8", A) and not t.contains("::1", A)
    t.insert("::/0", value=B)
    assert t.find("203.0.113.9") == A and t.find("2001:db8::1") == B
    t.insert("::ffff:10.0.0.0", 104, C)  # no v4-mapped handling: an IPv6 network, nothing else
    assert t.find("10.0.0.1") == A and t.find("::ffff:10.0.0.1") == C
    t.remove_value(A)
    assert t.find("203.0.113.9") is None and t.find("2001:db8::1") == B


def test_same_network_by_two_values_then_removal_of_the_later():
    t = AllowedIps()
    t.insert("10.0.0.0/8", value=C)
    t.insert("10.7.0.0/16", value=A)
    t.insert("10.7.0.0/16", value=B)
    assert t.find("10.7.1.1") == B
    assert t.contains("10.7.1.1", A) and t.contains("10.7.1.1", B)
    assert len(t) == 2
    t.remove_value(B)
    # the reference's quirk: the /16 has no route now (its route was B's), A still owns
    # it, and the /8's route shows through
    assert t.find("10.7.1.1") == C
    assert t.contains("10.7.1.1", A) and not t.contains("10.7.1.1", B)
    assert len(t) == 1
    t.remove_value(C)
    assert t.find("10.7.1.1") is None and t.contains("10.7.1.1", A)
    assert len(t) == 0


def test_find_and_contains_disagree_where_prefixes_nest():
    t = AllowedIps()
    t.insert("172.16.0.0/12", value=A)
    t.insert("172.17.0.0/16", value=B)
    assert t.find("172.17.5.5") == B
    assert t.contains("172.17.5.5", A) and t.contains("172.17.5.5", B)
    assert t.find("172.18.5.5") == A and not t.contains("172.18.5.5", B)


def test_clear_and_empty_table():
    t = AllowedIps()
    assert len(t) == 0
    assert t.find("1.2.3.4") is None and t.find("::1") is None
    assert not t.contains("1.2.3.4", 0) and not t.contains("::1", 0)
    t.insert("1.2.3.0/24", value=0)
    t.insert("fd00::/8", value=0)
    assert t.find("1.2.3.4") == 0 and t.contains("fd00::5", 0) and len(t) == 2
    t.clear()
    assert len(t) == 0
    assert t.find("1.2.3.4") is None and not t.contains("1.2.3.4", 0) and not t.contains("fd00::5", 0)
    t.insert("1.2.3.0/24", value=5)
    assert t.find("1.2.3.4") == 5


def test_accepts_str_bytes_and_ipaddress_objects():
    t = AllowedIps()
    t.insert(ipaddress.ip_network("198.51.100.0/24"), value=A)
    t.insert(ipaddress.IPv6Address("2001:db8:1::"), 48, B)
    for probe in ("198.51.100.7", ipaddress.IPv4Address("198.51.100.7"), bytes([198, 51, 100, 7])):
        assert t.find(probe) == A and t.contains(probe, A)
    p6 = ipaddress.IPv6Address("2001:db8:1:2::3")
    for probe in (str(p6), p6, p6.packed):
        assert t.find(probe) == B and t.contains(probe, B)
    with pytest.raises(ValueError):
        t.find(b"\x01\x02\x03")


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_tables_match_the_model(seed):
    """Interleaved inserts and removals (the image is rebuilt after each change that a
    lookup follows), then 2000 addresses: every find and every contains(addr, v) for all
    48 values equals the model's."""
    t, m = AllowedIps(), AM.Model()
    ta = AM.Adapter(t)
    ops = AM.random_ops(seed)
    third = len(ops) // 3
    for part in (ops[:third], ops[third:2 * third], ops[2 * third:]):
        AM.apply_ops(part, ta, m)
        for fam, a in AM.random_addresses(seed + 100, m, 200):  # (forces a rebuild mid-way)
            assert ta.find(fam, a) == m.find(fam, a)
    assert len(t) == len(m)
    addrs = AM.random_addresses(seed, m)
    assert len(addrs) == 2000
    shares = AM.check_shares(m, addrs)
    print("hit / miss / in two or more networks:", shares)
    for fam, a in addrs:
        assert ta.find(fam, a) == m.find(fam, a), (fam, hex(a))
        for v in range(AM.N_VALUES):
            assert ta.contains(fam, a, v) == m.contains(fam, a, v), (fam, hex(a), v)


def test_null_arguments_fail_loudly():
    lib = neptun_amd.load()
    buf = ctypes.create_string_buffer(16)
    v = ctypes.c_uint32()
    h = ctypes.c_void_p()
    assert lib.wg_allowed_create(None) == -1
    assert b"allowed_create" in lib.wg_gpu_last_error()
    assert lib.wg_allowed_insert(None, 4, buf, 8, 1) == -1
    assert b"allowed_insert: null" in lib.wg_gpu_last_error()
    assert lib.wg_allowed_create(ctypes.byref(h)) == 0
    assert lib.wg_allowed_insert(h, 4, None, 8, 1) == -1
    assert lib.wg_allowed_insert(h, 5, buf, 8, 1) == -1
    assert b"family" in lib.wg_gpu_last_error()
    assert lib.wg_allowed_remove_value(None, 1) == -1
    assert b"allowed_remove_value" in lib.wg_gpu_last_error()
    assert lib.wg_allowed_clear(None) == -1
    assert lib.wg_allowed_count(None) == 0
    assert lib.wg_allowed_find(None, 4, buf, ctypes.byref(v)) == -1
    assert lib.wg_allowed_find(h, 4, buf, None) == -1
    assert b"allowed_find: null" in lib.wg_gpu_last_error()
    assert lib.wg_allowed_contains(None, 4, buf, 1) == -1
    assert lib.wg_allowed_contains(h, 4, None, 1) == -1
    assert b"allowed_contains: null" in lib.wg_gpu_last_error()
    assert lib.wg_allowed_destroy(h) == 0 and lib.wg_allowed_destroy(None) == 0
    # the device and Tunn entry points refuse nulls before touching a GPU
    assert lib.wg_gpu_allowed_set(None, None) == -1
    assert b"allowed_set" in lib.wg_gpu_last_error()
    assert lib.wg_gpu_allowed_route_batch(None, None, 1, None, None, 1, None) == -1
    assert b"allowed_route_batch: null" in lib.wg_gpu_last_error()
    assert lib.wg_gpu_allowed_filter_batch(None, None, 1, None, None, None, 4, None, None) == -1
    assert b"allowed_filter_batch: null" in lib.wg_gpu_last_error()
    from neptun_amd.tunn import TunnResult, _bind
    _bind(lib)
    res = (TunnResult * 1)()
    assert lib.wg_tunn_encapsulate_routed(None, None, None, 0, 1, None, None, None, None, res, None) == -1
    assert b"encapsulate_routed: null" in lib.wg_gpu_last_error()
    assert lib.wg_tunn_decapsulate_multi_allowed(None, None, None, 0, 1, None, None, None, None, None, res) == -1
    assert b"decapsulate_multi_allowed: null" in lib.wg_gpu_last_error()
    assert lib.wg_gpu_abi_version() == 1


def test_tunn_kind_skipped_is_5():
    from neptun_amd import tunn
    text = open(neptun_amd.HEADER_PATH.replace("neptun_gpu.h", "neptun_tunn.h")).read()
    assert "WG_TUNN_SKIPPED = 5" in text and tunn.SKIPPED == 5
