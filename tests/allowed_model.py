"""Brute-force model of the AllowedIPs table (include/neptun_gpu.h wg_allowed_*) and
the randomised tables the CPU and GPU tests share.

Two dicts and integer masks, nothing else: `route` maps a network to its value (the
last insert wins, Device::peers_by_ip), `owned` maps a value to its networks
(Peer::allowed_ips).  A network is (family, network address as int, prefix length).
"""
import ipaddress
import random

NONE = 0xFFFFFFFF
BITS = {4: 32, 6: 128}


def mask(fam, cidr):
    return ((1 << cidr) - 1) << (BITS[fam] - cidr)


def to_bytes(fam, a):
    return a.to_bytes(BITS[fam] // 8, "big")


class Model:
    def __init__(self):
        self.route = {}
        self.owned = {}

    def insert(self, fam, addr, cidr, value):
        net = (fam, addr & mask(fam, cidr), cidr)  # host bits truncated
        self.route[net] = value
        self.owned.setdefault(value, set()).add(net)

    def remove_value(self, value):
        self.owned.pop(value, None)
        self.route = {n: v for n, v in self.route.items() if v != value}

    def clear(self):
        self.route, self.owned = {}, {}

    def __len__(self):
        return len(self.route)

    @staticmethod
    def covers(net, fam, addr):
        return net[0] == fam and (addr & mask(fam, net[2])) == net[1]

    def find(self, fam, addr):
        best = None
        for net, v in self.route.items():
            if self.covers(net, fam, addr) and (best is None or net[2] > best[0]):
                best = (net[2], v)
        return NONE if best is None else best[1]

    def contains(self, fam, addr, value):
        return any(self.covers(net, fam, addr) for net in self.owned.get(value, ()))

    def stored(self):
        return set(self.route) | {n for s in self.owned.values() for n in s}

    def depth(self, fam, addr):
        """stored networks (either relation) containing addr"""
        return sum(self.covers(net, fam, addr) for net in self.stored())


def dst_address(p):
    """Tunn::dst_address (noise/mod.rs:205-223): (family, int) or None."""
    if len(p) < 20:
        return None
    v = p[0] >> 4
    if v == 4:
        return 4, int.from_bytes(p[16:20], "big")
    if v == 6 and len(p) >= 40:
        return 6, int.from_bytes(p[24:40], "big")
    return None


def src_address(p):
    """the source address validate_decapsulated_packet reads (mod.rs:606-659)"""
    if len(p) < 20:
        return None
    v = p[0] >> 4
    if v == 4:
        return 4, int.from_bytes(p[12:16], "big")
    if v == 6 and len(p) >= 40:
        return 6, int.from_bytes(p[8:24], "big")
    return None


V4_LENS = [7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32]
V6_LENS = [7, 8, 9, 63, 64, 65, 120, 127, 128]
N_VALUES = 48


def random_ops(seed, networks=160):
    """The randomised table as a list of operations ("insert", fam, addr, cidr, value) /
    ("remove", value): about `networks` inserts, 60 % IPv4, over 48 values; after the
    first 40, half of the new networks are nested under one already inserted; value
    removals are interleaved (a removed value's networks are inserted again for others
    as the run goes on)."""
    rng = random.Random(seed)
    ops, nets = [], []
    for k in range(networks):
        fam = 4 if rng.random() < 0.6 else 6
        lens = V4_LENS if fam == 4 else V6_LENS
        parents = [n for n in nets if n[0] == fam and n[2] < BITS[fam]]
        if k >= 40 and parents and rng.random() < 0.5:
            pf, pa, pc = rng.choice(parents)
            longer = [c for c in lens if c > pc]
            cidr = rng.choice(longer) if longer else BITS[fam]
            addr = pa | (rng.getrandbits(BITS[fam]) & ~mask(fam, pc) & ((1 << BITS[fam]) - 1))
        else:
            cidr = rng.choice(lens)
            addr = rng.getrandbits(BITS[fam])
        value = rng.randrange(N_VALUES)
        ops.append(("insert", fam, addr, cidr, value))
        nets.append((fam, addr & mask(fam, cidr), cidr))
        if k % 23 == 22:
            ops.append(("remove", rng.randrange(N_VALUES)))
        if k % 31 == 30:  # a collision: another value inserts a network already there
            f, a, c = rng.choice(nets)
            ops.append(("insert", f, a, c, rng.randrange(N_VALUES)))
    return ops


def apply_ops(ops, *tables):
    """Run the operations on Model-like tables (Model, or AllowedIps through Adapter)."""
    for op in ops:
        for t in tables:
            if op[0] == "insert":
                t.insert(*op[1:])
            else:
                t.remove_value(op[1])


def random_addresses(seed, model, count=2000):
    """60 % under a stored network, 40 % uniform; [(fam, int)]"""
    rng = random.Random(seed * 7919 + 1)
    stored = sorted(model.stored())
    out = []
    for _ in range(count):
        if stored and rng.random() < 0.6:
            fam, a, c = rng.choice(stored)
            a |= rng.getrandbits(BITS[fam]) & ~mask(fam, c) & ((1 << BITS[fam]) - 1)
        else:
            fam = 4 if rng.random() < 0.6 else 6
            a = rng.getrandbits(BITS[fam])
        out.append((fam, a))
    return out


def check_shares(model, addrs):
    """The generator's cover of the cases, asserted on the MODEL's answers: at least
    40 % of the addresses hit a route, 20 % miss, 15 % lie in two or more networks."""
    n = len(addrs)
    hits = sum(model.find(f, a) != NONE for f, a in addrs)
    deep = sum(model.depth(f, a) >= 2 for f, a in addrs)
    assert hits >= 0.40 * n, (hits, n)
    assert n - hits >= 0.20 * n, (n - hits, n)
    assert deep >= 0.15 * n, (deep, n)
    return hits, n - hits, deep


class Adapter:
    """neptun_amd.AllowedIps behind the Model's (family, int) interface."""

    def __init__(self, table):
        self.t = table

    def insert(self, fam, addr, cidr, value):
        self.t.insert(to_bytes(fam, addr), cidr, value)

    def remove_value(self, value):
        self.t.remove_value(value)

    def find(self, fam, addr):
        v = self.t.find(to_bytes(fam, addr))
        return NONE if v is None else v

    def contains(self, fam, addr, value):
        return self.t.contains(to_bytes(fam, addr), value)


def ip_obj(fam, a):
    return ipaddress.IPv4Address(a) if fam == 4 else ipaddress.IPv6Address(a)
