"""AllowedIPs on the device and at the Tunn level against the brute-force model of
tests/allowed_model.py: wg_gpu_allowed_route_batch (outbound: longest-prefix match of
the destination address, device/mod.rs:1295-1313), wg_gpu_allowed_filter_batch
(inbound: peer.is_allowed_ip(source), device/mod.rs:1056), and the two routed Tunn
calls over oracle/tunn_model.py.
"""
import random
import struct

import numpy as np
import pytest

from oracle import pyoracle as o
from oracle import tunn_model as M

import allowed_model as AM
from test_tunn_gpu import Arena, check_same

pytestmark = pytest.mark.gpu

NONE = AM.NONE
SKIPPED = 5
BAD_KEY_SLOT = 101
LENGTHS = [0, 1, 19, 20, 39, 40, 60, 1350]
NIBBLES = [4, 4, 4, 6, 6, 0, 5, 15]


@pytest.fixture(scope="module")
def table():
    """The randomised table of the CPU test (seed 1) and its model."""
    from neptun_amd import AllowedIps
    t, m = AllowedIps(), AM.Model()
    AM.apply_ops(AM.random_ops(1), AM.Adapter(t), m)
    return t, m


def packets_for(seed, model, n):
    """n plaintext packets over LENGTHS x NIBBLES (so v4 headers shorter than 20 bytes
    and v6 headers shorter than 40 occur), the destination drawn like the CPU test's
    addresses and written where its family's header has it, whatever the nibble says."""
    rng = random.Random(seed)
    addrs = AM.random_addresses(seed + 5, model, n)
    out = []
    for k in range(n):
        ln = LENGTHS[k % len(LENGTHS)] if n >= 8 else rng.choice(LENGTHS[3:])
        nib = rng.choice(NIBBLES)
        fam, a = addrs[k]
        if nib in (4, 6):
            fam = nib
            if addrs[k][0] != fam:  # another family's draw: keep the hit / miss mix
                fam, a = next(((f, x) for f, x in addrs[k:] + addrs[:k] if f == nib), (nib, 0))
        b = bytearray(rng.randbytes(ln))
        if ln:
            b[0] = nib << 4 | rng.randrange(16)
        at = 16 if fam == 4 else 24
        raw = AM.to_bytes(fam, a)
        if ln >= at + len(raw):
            b[at:at + len(raw)] = raw
        out.append(bytes(b))
    return out


def pack(rng, pkts, align=1):
    """Packets at byte offsets that include odd ones (align 1) -> (buffer, offsets)."""
    offs, at = [], 0
    for p in pkts:
        at += rng.choice([0, 1, 2, 3, 5, 8]) if align == 1 else 0
        at = (at + align - 1) // align * align
        offs.append(at)
        at += len(p)
    buf = np.zeros(at + 64, np.uint8)
    for off, p in zip(offs, pkts):
        buf[off:off + len(p)] = np.frombuffer(p, np.uint8)
    return buf, offs


def descs_for(rng, pkts, offs, key_slot=0xABCD):
    d = np.zeros(len(pkts), o.DESC_DTYPE)
    d["src_off"] = offs
    d["dst_off"] = [rng.getrandbits(40) for _ in pkts]
    d["counter"] = [rng.getrandbits(64) for _ in pkts]
    d["len"] = [len(p) for p in pkts]
    d["key_slot"] = key_slot
    return d


def dev(torch, a):
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def route(torch, gpu, descs, buf, set_key_slot=True, with_values=True):
    n = len(descs)
    d_descs, d_src = dev(torch, descs), dev(torch, buf)
    d_val = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if with_values else None
    gpu.allowed_route_batch(d_descs, n, d_src, d_val, set_key_slot)
    torch.cuda.synchronize()
    back = d_descs.cpu().numpy().view(o.DESC_DTYPE)
    vals = d_val.cpu().numpy().view(np.uint32) if with_values else None
    return back, vals


def expected_values(model, pkts):
    out = []
    for p in pkts:
        a = AM.dst_address(p)
        out.append(NONE if a is None else model.find(*a))
    return np.array(out, np.uint32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 2000])
def test_route_batch_matches_the_model(torch_cuda, gpu, table, n):
    t, m = table
    rng = random.Random(n)
    pkts = packets_for(100 + n, m, n)
    buf, offs = pack(rng, pkts)
    descs = descs_for(rng, pkts, offs)
    want = expected_values(m, pkts)
    gpu.allowed_set(t)
    try:
        back, vals = route(torch_cuda, gpu, descs, buf)
    finally:
        gpu.allowed_set(None)
    assert np.array_equal(vals, want)
    assert np.array_equal(back["key_slot"], want)
    for f in ("src_off", "dst_off", "counter", "len"):
        assert np.array_equal(back[f], descs[f]), f
    if n == 2000:
        assert any(off % 2 for off in offs) and any(off % 4 == 0 for off in offs)
        with_addr = [AM.dst_address(p) for p in pkts]
        assert sum(a is None for a in with_addr) >= n // 4  # short headers, other nibbles
        shares = AM.check_shares(m, [a for a in with_addr if a is not None])
        print("hit / miss / in two or more networks:", shares)
        short4 = sum(len(p) and p[0] >> 4 == 4 and len(p) < 20 for p in pkts)
        short6 = sum(len(p) and p[0] >> 4 == 6 and len(p) < 40 for p in pkts)
        assert short4 >= 20 and short6 >= 20


def test_route_batch_without_an_image_changed_image_and_untouched_descriptors(torch_cuda, gpu, table):
    from neptun_amd import AllowedIps
    t, m = table
    rng = random.Random(9)
    pkts = packets_for(77, m, 300)
    buf, offs = pack(rng, pkts)
    descs = descs_for(rng, pkts, offs)
    gpu.allowed_set(None)
    back, vals = route(torch_cuda, gpu, descs, buf)
    assert (vals == NONE).all() and (back["key_slot"] == NONE).all()
    try:
        gpu.allowed_set(t)
        want = expected_values(m, pkts)
        # set_key_slot = 0: the descriptors stay bit-identical, the values are still written
        back, vals = route(torch_cuda, gpu, descs, buf, set_key_slot=False)
        assert back.tobytes() == descs.tobytes()
        assert np.array_equal(vals, want)
        # no value_out: only the key slots
        back, _ = route(torch_cuda, gpu, descs, buf, with_values=False)
        assert np.array_equal(back["key_slot"], want)
        # a changed table: the device follows it from the next allowed_set on
        t2, m2 = AllowedIps(), AM.Model()
        AM.apply_ops(AM.random_ops(1), AM.Adapter(t2), m2)
        gone = [v for v in range(AM.N_VALUES) if v in m2.owned][:6]
        for x in (AM.Adapter(t2), m2):
            for v in gone:
                x.remove_value(v)
            x.insert(4, 0, 0, 4242)  # a default route
        want2 = expected_values(m2, pkts)
        assert not np.array_equal(want2, want)
        back, vals = route(torch_cuda, gpu, descs, buf)
        assert np.array_equal(vals, want)  # (t2 is not on the device yet)
        gpu.allowed_set(t2)
        back, vals = route(torch_cuda, gpu, descs, buf)
        assert np.array_equal(vals, want2) and np.array_equal(back["key_slot"], want2)
    finally:
        gpu.allowed_set(None)


def v4_packet(rng, total, src, dst):
    b = bytearray(rng.randbytes(total))
    b[0] = 0x45
    b[2:4] = struct.pack(">H", total)
    b[12:16] = bytes(src)
    b[16:20] = bytes(dst)
    return bytes(b)


def v6_packet(rng, total, src, dst):
    b = bytearray(rng.randbytes(total))
    b[0] = 0x60
    b[4:6] = struct.pack(">H", total - 40)
    b[8:24] = bytes(src)
    b[24:40] = bytes(dst)
    return bytes(b)


def seal_case(rng):
    """8 key slots 1000..1007 as the values of a small table, 96 packets, the model's routes"""
    from neptun_amd import AllowedIps
    t, m = AllowedIps(), AM.Model()
    for k in range(8):
        for x in (AM.Adapter(t), m):
            x.insert(4, (10 << 24) | (k << 16), 16, 1000 + k)
            x.insert(6, (0xfd00 + k) << 112, 16, 1000 + k)
    for x in (AM.Adapter(t), m):
        x.insert(4, (10 << 24) | (3 << 16) | (9 << 8), 24, 1005)  # nested in slot 1003's /16
    pkts = []
    for i in range(96):
        r = rng.random()
        ln = rng.choice([20, 40, 60, 61, 200, 1350])
        if r < 0.55:
            pkts.append(v4_packet(rng, ln, rng.randbytes(4), [10, rng.randrange(10), rng.choice([9, 200]), 7]))
        elif r < 0.8:
            pkts.append(v6_packet(rng, max(ln, 40), rng.randbytes(16),
                                  struct.pack(">H", 0xfd00 + rng.randrange(10)) + rng.randbytes(14)))
        else:
            pkts.append(bytes([rng.choice([0x05, 0x75, 0x45])]) + rng.randbytes(rng.randrange(0, 19)))
    buf, offs = pack(rng, pkts, align=16)
    descs = descs_for(rng, pkts, offs)
    descs["counter"] = np.arange(len(pkts)) + 7
    dst_offs, at = [], 0
    for p in pkts:
        dst_offs.append(at)
        at += (len(p) + 32 + 15) // 16 * 16
    descs["dst_off"] = dst_offs
    want = expected_values(m, pkts)
    assert (want == NONE).sum() >= 10 and (want == 1005).sum() >= 2 and len(set(want.tolist())) >= 8
    return t, pkts, buf, descs, dst_offs, at, want


def test_route_then_seal(torch_cuda, gpu):
    """Key slots as values: allowed_route_batch fills key_slot, seal_batch seals the
    routed packets under the routed key and answers the others with BAD_KEY_SLOT."""
    torch = torch_cuda
    rng = random.Random(5)
    keys = np.frombuffer(rng.randbytes(8 * 32), np.uint8).reshape(8, 32)
    idx = np.array([rng.getrandbits(32) for _ in range(8)], np.uint32)
    gpu.set_keys(1000, keys, idx)
    t, pkts, buf, descs, dst_offs, at, want = seal_case(rng)
    n = len(pkts)
    d_descs, d_src = dev(torch, descs), dev(torch, buf)
    d_dst = torch.full((at + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    gpu.allowed_set(t)
    try:
        gpu.allowed_route_batch(d_descs, n, d_src, None, True)
        gpu.seal_batch(d_descs, n, d_src, d_dst, d_st)
        torch.cuda.synchronize()
    finally:
        gpu.allowed_set(None)
    st, out = d_st.cpu().numpy(), d_dst.cpu().numpy()
    for i, p in enumerate(pkts):
        lo, hi = dst_offs[i], dst_offs[i] + len(p) + 32
        if want[i] == NONE:
            assert st[i] == BAD_KEY_SLOT, i
            assert (out[lo:hi] == 0xEE).all(), i
        else:
            k = int(want[i]) - 1000
            assert st[i] == 0, (i, st[i])
            assert out[lo:hi].tobytes() == o.format_packet_data(keys[k].tobytes(), int(idx[k]), i + 7, p), i


def test_open_then_filter(torch_cuda, gpu):
    """~300 datagrams of 8 peers (receiving keys in slots 16 p, so key_slot >> 4 is the
    peer): allowed_out == the model's contains(source, peer) on packets that opened, 0
    on tampered ones, keepalives and plaintexts without a source address."""
    torch = torch_cuda
    rng = random.Random(6)
    P = 8
    keys = [rng.randbytes(32) for _ in range(P)]
    idx = [rng.getrandbits(32) for _ in range(P)]
    for p in range(P):
        gpu.set_keys(16 * p, np.frombuffer(keys[p], np.uint8), np.array([idx[p]], np.uint32))
    t, m, who, plain, kind = filter_case(rng, keys, idx)
    dgs = [k[1] for k in kind]
    buf, offs = pack(rng, dgs, align=16)
    descs = descs_for(rng, dgs, offs)
    descs["dst_off"] = offs  # plaintext i where datagram i starts, in a buffer of its own
    descs["key_slot"] = [16 * p for p in who]
    n = len(dgs)
    d_descs, d_src = dev(torch, descs), dev(torch, buf)
    d_dst = torch.full((len(buf),), 0xEE, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_expect = torch.from_numpy(np.array(who, np.int32)).cuda()
    gpu.open_batch(d_descs, n, d_src, d_dst, d_st)
    torch.cuda.synchronize()
    st = d_st.cpu().numpy()
    want = []
    for i in range(n):
        assert (st[i] == 0) == (not kind[i][0]), (i, st[i])
        want.append(filter_want(m, plain[i], who[i]) if st[i] == 0 else 0)
    want = np.array(want, np.uint8)
    assert 0.25 * n < want.sum() < 0.75 * n
    filter_rest(torch, gpu, t, m, n, P, who, plain, st, want, d_descs, d_dst, d_st, d_expect)


def filter_want(m, pt, value):
    a = AM.src_address(pt)
    return 1 if a is not None and m.contains(a[0], a[1], value) else 0


def filter_case(rng, keys, idx):
    from neptun_amd import AllowedIps
    P = len(keys)
    t, m = AllowedIps(), AM.Model()
    for p in range(P):
        for x in (AM.Adapter(t), m):
            x.insert(4, (10 << 24) | (p << 16), 16, p)                       # its own /16
            x.insert(4, (10 << 24) | (((p + 1) % P) << 16) | (77 << 8), 24, p)  # inside the neighbour's
            x.insert(6, (0xfd00 + p) << 112, 32, p)
    who, plain, kind = [], [], []
    for i in range(304):
        p = rng.randrange(P)
        r = rng.random()
        if r < 0.3:    # from its own network
            pt = v4_packet(rng, rng.choice([20, 21, 64, 300]), [10, p, rng.randrange(256), 1], rng.randbytes(4))
        elif r < 0.45:  # from another peer's network
            pt = v4_packet(rng, 48, [10, (p + 3) % P, rng.choice([5, 77]), 1], rng.randbytes(4))
        elif r < 0.6:  # from the /24 it owns inside the neighbour's /16, or the neighbour from there
            q = rng.choice([p, (p + 1) % P])
            pt = v4_packet(rng, 60, [10, (p + 1) % P, 77, 9], rng.randbytes(4))
            p = q
        elif r < 0.75:
            pt = v6_packet(rng, rng.choice([40, 41, 120]), struct.pack(">HH", 0xfd00 + rng.choice([p, (p + 1) % P]), 0)
                           + rng.randbytes(12), rng.randbytes(16))
        elif r < 0.8:
            pt = v4_packet(rng, 33, [11, p, 0, 1], rng.randbytes(4))  # no network at all
        elif r < 0.87:
            pt = b""  # keepalive
        elif r < 0.94:  # no source address: v4 nibble below 20 bytes, v6 below 40, neither
            pt = rng.choice([bytes([0x45]) + rng.randbytes(18), bytes([0x60]) + rng.randbytes(38),
                             bytes([0x75]) + rng.randbytes(59)])
        else:
            pt = v4_packet(rng, 64, [10, p, 1, 1], rng.randbytes(4))
        d = bytearray(o.format_packet_data(keys[p], idx[p], i, pt))
        tampered = r >= 0.94
        if tampered:
            d[rng.randrange(16, len(d))] ^= 0x10
        who.append(p)
        plain.append(pt)
        kind.append((tampered, bytes(d)))
    return t, m, who, plain, kind


def filter_rest(torch, gpu, t, m, n, P, who, plain, st, want, d_descs, d_dst, d_st, d_expect):
    try:
        for label, image in (("no image", None), ("image", t)):
            gpu.allowed_set(image)
            for expect, shift in ((d_expect, 0), (None, 4)):
                d_ok = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
                gpu.allowed_filter_batch(d_descs, n, d_dst, d_st, d_ok, expect, shift)
                torch.cuda.synchronize()
                got = d_ok.cpu().numpy()
                assert np.array_equal(got, want if image is not None else np.zeros(n, np.uint8)), (label, shift)
        # a wrong expectation: every peer checked against its neighbour's networks
        other = np.array([(p + 1) % P for p in who], np.int32)
        d_ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
        gpu.allowed_filter_batch(d_descs, n, d_dst, d_st, d_ok, torch.from_numpy(other).cuda(), 0)
        torch.cuda.synchronize()
        want2 = [filter_want(m, plain[i], int(other[i])) if st[i] == 0 else 0 for i in range(n)]
        assert np.array_equal(d_ok.cpu().numpy(), np.array(want2, np.uint8))
    finally:
        gpu.allowed_set(None)


# --- Tunn level ---------------------------------------------------------------------

N_PEERS = 6
FIRST = 2000  # key slots of the session context used here: [2000, 2000 + 2 * 6 * 16)


def tunn_setup(rng, eng):
    """6 peers, each a sending side A_p and the mirror receiving side B_p (model and GPU),
    and the table: peer p owns 10.p.0.0/16 and 10.(p+1).50.0/24 inside its neighbour's
    /16; peer 0 also fd00::/16; one network routes to a value that names no peer."""
    from neptun_amd import AllowedIps
    a_side, b_side = [], []
    for p in range(N_PEERS):
        k1, k2 = rng.randbytes(32), rng.randbytes(32)
        ia, ib = 101 + 8 * p, 202 + 8 * p
        am, ag = M.Tunn(), eng.tunn(FIRST + 16 * p)
        bm, bg = M.Tunn(), eng.tunn(FIRST + 16 * (N_PEERS + p))
        for x in (am, ag):
            x.install_session(ia, ib, k2, k1, True)
        for x in (bm, bg):
            x.install_session(ib, ia, k1, k2, True)
        a_side.append((am, ag, [(ia, ib, k2, k1)]))
        b_side.append((bm, bg, [(ib, ia, k1, k2)]))
    t, m = AllowedIps(), AM.Model()
    for x in (AM.Adapter(t), m):
        for p in range(N_PEERS):
            x.insert(4, (10 << 24) | (p << 16), 16, p)
            x.insert(4, (10 << 24) | (((p + 1) % N_PEERS) << 16) | (50 << 8), 24, p)
        x.insert(6, 0xfd00 << 112, 16, 0)
        x.insert(4, (10 << 24) | (200 << 16), 16, 99)  # a route to no peer
    return a_side, b_side, t, m


def check_state(pairs):
    for tm, tg, ses in pairs:
        for local, *_ in ses:
            ctr, w = tg.session_counters(local % M.N_SESSIONS)
            sm = tm.sessions[local % M.N_SESSIONS]
            assert ctr == sm.sending_counter
            assert w.next == sm.window.next and list(w.bitmap) == sm.window.bitmap
            assert w.receive_cnt == sm.window.receive_cnt
        assert tg.stats() == (tm.tx_bytes, tm.rx_bytes)


def outbound(rng, n):
    out = []
    for _ in range(n):
        p = rng.randrange(N_PEERS)
        r = rng.random()
        src = ([10, p, rng.randrange(256), 2] if rng.random() < 0.6 else          # own network
               [10, (p + 1) % N_PEERS, 50, 3] if rng.random() < 0.5 else          # its nested /24
               [10, (p + 2) % N_PEERS, rng.choice([50, 8]), 4])                   # spoofed
        ln = rng.choice([20, 64, 576, 1350, rng.randrange(20, 1400)])
        if r < 0.5:
            out.append(v4_packet(rng, ln, src, [10, p, rng.randrange(256), 1]))
        elif r < 0.65:  # routed by the /24 inside the neighbour's /16
            out.append(v4_packet(rng, ln, src, [10, (p + 1) % N_PEERS, 50, rng.randrange(256)]))
        elif r < 0.72:
            out.append(v6_packet(rng, max(ln, 40), struct.pack(">H", 0xfd00) + rng.randbytes(14),
                                 struct.pack(">H", 0xfd00) + rng.randbytes(14)))
        elif r < 0.8:
            out.append(v4_packet(rng, ln, src, [172, 16, 0, 1]))     # no route
        elif r < 0.85:
            out.append(v4_packet(rng, ln, src, [10, 200, 0, 1]))     # value 99: no such peer
        elif r < 0.9:
            out.append(v6_packet(rng, 60, rng.randbytes(16), b"\x20\x01" + rng.randbytes(14)))  # no route
        elif r < 0.95:
            out.append(bytes([0x45]) + rng.randbytes(rng.randrange(0, 19)))  # no address
        else:
            out.append(b"" if rng.random() < 0.5 else bytes([0x75]) + rng.randbytes(40))
    return out


def model_routed(m, a_side, srcs, dsts):
    res, vals = [], []
    for s, d in zip(srcs, dsts):
        a = AM.dst_address(s)
        v = NONE if a is None else m.find(*a)
        vals.append(v)
        res.append(a_side[v][0].encapsulate(s, d) if v < N_PEERS else (SKIPPED, 0, 0))
    return res, np.array(vals, np.uint32)


def model_filtered(m, b_side, vals, dgs, dsts):
    res = []
    for v, d, x in zip(vals, dgs, dsts):
        r = b_side[v][0].decapsulate(d, x)
        if r[0] == M.WRITE_TO_TUNNEL and not m.contains(r[3], int.from_bytes(r[4], "big"), int(v)):
            r = (SKIPPED,) + tuple(r[1:])
        res.append(r)
    return res


@pytest.mark.parametrize("registered", [False, True])
def test_routed_tunn_calls_match_the_model(gpu, registered):
    from neptun_amd import Engine
    from neptun_amd import tunn as T
    rng = random.Random(40 + registered)
    eng = Engine(gpu)
    a_side, b_side, t, m = tunn_setup(rng, eng)
    peers_a = [x[1] for x in a_side]
    peers_b = [x[1] for x in b_side]
    windows = []
    try:
        for n in (50, 600):
            srcs = outbound(rng, n)
            caps = [len(s) + 32 + rng.randrange(0, 3) * 16 if rng.random() > 0.04 else len(s) + 16 for s in srcs]
            dm = [bytearray(b"\xee" * c) for c in caps]
            res_m, val_m = model_routed(m, a_side, srcs, dm)
            if registered:
                a_src, a_dst = Arena(srcs, [0] * n), Arena([b""] * n, caps)
                for a in (a_src, a_dst):
                    gpu.register_host(*a.window())
                    windows.append(a.window()[0])
                res_g, val_g = eng.encapsulate_routed_ptrs(t, peers_a, a_src.ptrs, a_src.lens, a_dst.ptrs,
                                                           np.array(caps, np.uint32))
                dg = [bytearray(a_dst.get(k, caps[k])) for k in range(n)]
            else:
                dg = [bytearray(b"\xee" * c) for c in caps]
                res_g, val_g = eng.encapsulate_routed(t, peers_a, srcs, dg)
            assert np.array_equal(val_g, val_m)
            check_same(res_g, res_m, dg, dm, f"routed encap {n}")
            kinds = [r[0] for r in res_m]
            assert kinds.count(SKIPPED) >= n // 8 and kinds.count(M.WRITE_TO_NETWORK) >= n // 2
            check_state(a_side)  # (the skipped packets took no counter and no tx_bytes)

            # inbound on the mirror side: the datagrams just made (own, nested and spoofed
            # sources), then replays of some and tampered copies of others
            sent = [(int(v), bytes(d[:r[2]])) for v, d, r in zip(val_m, dm, res_m) if r[0] == M.WRITE_TO_NETWORK]
            extra = []
            for v, d in rng.sample(sent, len(sent) // 6):
                if rng.random() < 0.5:
                    extra.append((v, d))  # a replay
                else:
                    b = bytearray(d)
                    b[rng.randrange(16, len(b))] ^= 4
                    extra.append((v, bytes(b)))
            inbound = sent + extra
            vals = np.array([v for v, _ in inbound], np.uint32)
            dgs = [d for _, d in inbound]
            caps = [max(len(d) - 16, 1) for d in dgs]
            dm = [bytearray(b"\xee" * c) for c in caps]
            res_m = model_filtered(m, b_side, vals, dgs, dm)
            if registered:
                a_in, a_out = Arena(dgs, [0] * len(dgs)), Arena([b""] * len(dgs), caps)
                for a in (a_in, a_out):
                    gpu.register_host(*a.window())
                    windows.append(a.window()[0])
                res_g = eng.decapsulate_multi_allowed_ptrs(t, peers_b, vals, a_in.ptrs, a_in.lens, a_out.ptrs,
                                                           np.array(caps, np.uint32))
                dg = [bytearray(a_out.get(k, caps[k])) for k in range(len(dgs))]
            else:
                dg = [bytearray(b"\xee" * c) for c in caps]
                res_g = eng.decapsulate_multi_allowed(t, peers_b, vals, dgs, dg)
            check_same(res_g, res_m, dg, dm, f"filtered decap {n}")
            for g, w in zip(res_g, res_m):
                if w[0] == SKIPPED:  # len, ip_version and src_ip are kept
                    assert g[3] == w[3] and g[4][:len(w[4])] == w[4]
            kinds = [r[0] for r in res_m]
            assert kinds.count(SKIPPED) >= len(dgs) // 20 and kinds.count(M.WRITE_TO_TUNNEL) >= len(dgs) // 3
            assert kinds.count(M.ERR) >= 2
            check_state(b_side)  # replay windows and rx_bytes: those of the unfiltered model run

        # an all-skipped batch is fine and consumes nothing
        srcs = [v4_packet(rng, 40, [10, 0, 0, 1], [192, 0, 2, k]) for k in range(30)] + [b"", b"\x45"]
        dg = [bytearray(b"\xee" * 100) for _ in srcs]
        res_g, val_g = eng.encapsulate_routed(t, peers_a, srcs, dg)
        assert all(r[:3] == (SKIPPED, 0, 0) for r in res_g) and (val_g == NONE).all()
        assert all(bytes(d) == b"\xee" * 100 for d in dg)
        check_state(a_side)
        if not registered:
            # the engine-free forms
            srcs = outbound(rng, 50)
            caps = [len(s) + 32 for s in srcs]
            dm = [bytearray(b"\xee" * c) for c in caps]
            dg = [bytearray(b"\xee" * c) for c in caps]
            res_m, val_m = model_routed(m, a_side, srcs, dm)
            res_g, val_g = T.encapsulate_routed(t, peers_a, srcs, dg)
            assert np.array_equal(val_g, val_m)
            check_same(res_g, res_m, dg, dm, "routed encap, no engine")
            sent = [(int(v), bytes(d[:r[2]])) for v, d, r in zip(val_m, dm, res_m) if r[0] == M.WRITE_TO_NETWORK]
            vals = np.array([v for v, _ in sent], np.uint32)
            dgs = [d for _, d in sent]
            dm = [bytearray(b"\xee" * len(d)) for d in dgs]
            dg = [bytearray(b"\xee" * len(d)) for d in dgs]
            check_same(T.decapsulate_multi_allowed(t, peers_b, vals, dgs, dg),
                       model_filtered(m, b_side, vals, dgs, dm), dg, dm, "filtered decap, no engine")
            check_state(a_side)
            check_state(b_side)
            # a value that names no peer is refused before anything runs
            from neptun_amd import NeptunGpuError
            with pytest.raises(NeptunGpuError, match="names no peer"):
                eng.decapsulate_multi_allowed(t, peers_b, [N_PEERS], dgs[:1], [bytearray(64)])
            check_state(b_side)
    finally:
        for w in windows:
            gpu.unregister_host(w)
        for _, tg, _ in a_side + b_side:
            tg.close()
        eng.close()
