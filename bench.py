#!/usr/bin/env python3
"""bench.py -- device-resident ChaCha20-Poly1305 seal+open throughput (BASELINE.json).

One step = one pass of the hot path over one batch: seal 1M x 1350 B packets
(Session::format_packet_data semantics, session.rs:205-259) then open the
resulting 1M datagrams (receive_packet_data, session.rs:265-302), all in HBM
(BASELINE config 2 per GPU; with --gpus 8 it is config 5: 8M packets, 1M per
GPU, contiguous shards, no collective on the data path -> "scaling": "weak").

    python bench.py [--gpus N] [--steps K] [--warmup W]   (N > 1: starts N ranks itself)
    torchrun --nproc-per-node N bench.py --gpus N ...   (one process per GPU; N must match)
    python bench.py --config 3|4   (supplementary lines for DESIGN.md)
    python bench.py --full   (the line with everything else: see below)
    python bench.py --dump-outputs DIR   (what the last timed step computed, as .npy)

Rank 0 prints one JSON line.  value = Gbit/s of plaintext round-trip goodput
over all ranks = sum_ranks(payload bytes per step) * 8 * K / max_rank(time of
K steps).

A plain run sets up, warms up, times the K steps and prints the line with the
figures those steps give (value, ms_per_step, per-kernel times, HBM fractions).
--full adds what takes work of its own: the verification of the timed batch
(statuses, whole-batch round trip, the OpenSSL EVP sample), the sustained steps
with power and clock sampling (and the roofline figures priced at that clock),
and the CPU baseline.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "Gbit/s device-resident ChaCha20-Poly1305 seal+open, 1350B pkts, 1/2/4/8 GPU"
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md chip table)


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    # (100 untimed steps, ~0.15 s: the package power controller clamps the clock for ~25
    # steps after a cold start and then settles; the timed steps are the
    # steady state a loaded gateway runs at)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--config", type=int, default=2, choices=(2, 3, 4))
    ap.add_argument("--full", action="store_true",
                    help="also verify the timed batch (statuses, round trip, EVP sample), run the "
                         "sustained steps with power sampling and the CPU baseline; the options "
                         "below that tune those legs only matter with it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last one computed as DIR/<name>.npy "
                         "(float32 / float64; a fixed seeded sample of the packets, at most 64 MB)")
    ap.add_argument("--packets", type=int, default=0,
                    help="config 2: packets per GPU (0 = 1M at 1350 B; other --size values keep the "
                         "same payload bytes per step, 1M x 1350 B, rounded to whole 512-packet groups)")
    ap.add_argument("--size", type=int, default=1350)
    ap.add_argument("--op", default="roundtrip", choices=("roundtrip", "seal", "open"),
                    help="config 2: what one step runs -- seal then open (BASELINE's headline), or only "
                         "the seal (the reference's own AEAD bench, chacha20poly1305_benching.rs:37-55) "
                         "or only the open of a batch sealed before timing")
    ap.add_argument("--stride", type=int, default=0, help="config 2 slot stride (0 = round up to 128)")
    ap.add_argument("--layout", default="slots", choices=("slots", "neptun"),
                    help="config 2 buffers: 'slots' = datagram at slot+0 / plaintext at slot+16 on both "
                         "sides with slot padding (the fast layout); 'neptun' = NepTUN's own layouts: "
                         "seal in place (device/mod.rs:1297-1337), open into a fresh buffer at offset 0 "
                         "(device/mod.rs:1140-1148), no slot padding")
    ap.add_argument("--per-size", type=int, default=1 << 18, help="config 3: packets per size")
    ap.add_argument("--mixed-sizes", default="64,256,576,1350,8900",
                    help="config 3: the payload sizes mixed (diagnostics; BASELINE's set by default)")
    ap.add_argument("--peers", type=int, default=4096, help="config 4")
    ap.add_argument("--per-peer", type=int, default=4096, help="config 4")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-slot-padding", action="store_true",
                    help="config 2: leave the slot bytes past each output untouched")
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="0 = one per physical core of this job's CPU share "
                         "(min of affinity, physical cores, OMP_NUM_THREADS)")
    ap.add_argument("--cpu-curve", default="1,2,4,8",
                    help="extra thread counts timed for the CPU baseline's scaling curve (capped by "
                         "the thread count above; empty = none)")
    ap.add_argument("--sustain-seconds", type=float, default=2.0,
                    help="N=1: extra seconds of steps after the timed region, reported apart as "
                         "'sustained' (the power-capped steady state; never the headline value)")
    ap.add_argument("--evp-sample", type=int, default=257,
                    help="sealed datagrams compared byte for byte against OpenSSL EVP")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1 (the line is the time of the timed steps)")
    return args


# ---------------------------------------------------------------------------
# --dump-outputs: the packets whose bytes are written are a seeded sample (the
# same packets for the same arguments), sized so a dump stays under 64 MB
# ---------------------------------------------------------------------------
DUMP_SEED = 0x44554D50  # "DUMP"
DUMP_PACKET_BYTES = 40_000_000  # float32 bytes of the sampled datagrams + plaintexts
DUMP_STATUS_BYTES = 16_000_000  # float32 bytes of the two status arrays when written whole


def dump_rows(sizes, budget: int = DUMP_PACKET_BYTES):
    """Sorted indices of the sampled packets: a seeded permutation's longest prefix whose
    datagrams (P + 32) and plaintexts (P), one float32 per byte, fit in `budget`."""
    import numpy as np
    sizes = np.asarray(sizes, np.int64)
    perm = np.random.default_rng(DUMP_SEED).permutation(len(sizes))
    cost = np.cumsum(4 * (2 * sizes[perm] + 32))
    return np.sort(perm[:int(np.searchsorted(cost, budget, side="right"))])


def to_host(t):
    """Device tensor -> numpy, through a pinned buffer (a copy engine write into
    locked pageable memory is the path DESIGN.md §6 keeps big copies off)."""
    import torch
    if not t.is_cuda:
        return t.numpy()
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t)
    torch.cuda.synchronize(t.device)
    return host.numpy().copy()


def dump_statuses(rows, **st):
    """The status arrays whole while both fit in DUMP_STATUS_BYTES, else at `rows`."""
    import torch
    n = len(next(iter(st.values())))
    if 4 * n * len(st) > DUMP_STATUS_BYTES:
        sel = torch.from_numpy(rows).to(next(iter(st.values())).device)
        return {f"{k}_sampled": to_host(v[sel].float()) for k, v in st.items()}
    return {k: to_host(v.float()) for k, v in st.items()}


def dump_outputs(wl, outdir: str, rank: int, world: int) -> dict:
    """Write wl.outputs() (name -> float32 / float64 array) as outdir/<name>.npy; with more
    than one rank each writes its own shard as <name>.rank<r>.npy."""
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    total, names = 0, []
    for name, a in wl.outputs().items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        fn = f"{name}.npy" if world == 1 else f"{name}.rank{rank}.npy"
        np.save(os.path.join(outdir, fn), a)
        total += a.nbytes
        names.append(fn)
    assert total <= 64_000_000, f"--dump-outputs wrote {total} bytes"
    return {"dir": outdir, "files": names, "bytes": total}


# ---------------------------------------------------------------------------
# workloads: each has .step(stream, evs) (events: before seal, between, after
# open), .verify() -> bool, .outputs() -> {name: array} (what the last step left,
# for --dump-outputs), .packets, .payload_bytes, .launch_bytes
# {seal, open}, .kernels {seal, open} (rocprof names), .describe() -> dict
# ---------------------------------------------------------------------------
class StridedWorkload:
    """Config 2 / 5: one session, uniform 1350 B, counters = base + lane index.

    layout "slots": plaintext at slot+16 (NepTUN's WG_HEADER_OFFSET, device/mod.rs:76)
    sealed into a separate wire buffer (datagram at slot+0) and opened back to
    slot+16, with slot padding -- both sides 128-byte-run aligned.
    layout "neptun": the buffers NepTUN itself hands to Tunn -- encapsulate_in_place
    seals the TUN buffer in place (plaintext at +16, datagram written over it at
    +0, device/mod.rs:1297-1337) and decapsulate opens the UDP buffer into a fresh
    buffer at offset 0 (device/mod.rs:1140-1148, the text-grid open); no padding."""

    def __init__(self, args, dev, rank, world):
        import numpy as np
        import torch

        import neptun_amd
        from tools import synth
        self.n, self.P = n, P = packets_for(args), args.size
        self.op = getattr(args, "op", "roundtrip")
        S = args.stride or synth.round_up(P + 32, 128)
        if S % 16 or S < P + 32:
            raise SystemExit("--stride must be a multiple of 16 and hold P + 32 bytes")
        self.S = S
        self.layout = getattr(args, "layout", "slots")
        self.ctx = neptun_amd.GpuContext(dev.index, key_slots=1)
        self.ctx.set_keys(0, synth.keys(1), np.array([synth.RECEIVER_IDX], np.uint32))
        # the slots' padding past each output is scratch here (as in NepTUN's
        # MAX_PKT_SIZE buffers): outputs are zero-filled to their 128-byte line end
        self.pad = not args.no_slot_padding and self.layout == "slots"
        self.ctx.set_slot_padding(self.pad)
        # shard: rank r owns packets [r*n, (r+1)*n) of the global batch; counters follow
        self.counter_base = rank * n
        # NepTUN slot layout (WG_HEADER_OFFSET = 16, device/mod.rs:76): plaintext 16
        # bytes into each slot, the datagram at the slot start -- both run-aligned
        self.pt = synth.device_payloads(n, P, S, dev, seed=synth.SEED + rank, offset=16)
        if self.layout == "neptun":
            # the TUN buffers: sealed in place, so each step re-seals what the last
            # one left there (same work); verify() restores them from self.pt first
            self.wire = self.pt.clone()
            self.open_off = 0
        else:
            self.wire = torch.zeros(n * S, dtype=torch.uint8, device=dev)
            self.open_off = 16
        self.back = torch.zeros(n * S, dtype=torch.uint8, device=dev)
        self.st_seal = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.st_open = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.packets = n
        self.payload_bytes = n * P
        # algorithmic HBM bytes per launch: seal reads P, writes P+32; open the reverse
        self.launch_bytes = {"seal": n * (2 * P + 32), "open": n * (2 * P + 32)}
        self.kernels = {"seal": "aead_strided_kernel<true, false>",
                        "open": "aead_strided_open_text_kernel" if self.layout == "neptun"
                        else "aead_strided_kernel<false, false>"}
        # under-filled grids of long packets run split waves (wg_gpu_ctx_set_split):
        # the split kernel + the finish kernel, both inside the timed launch
        ks = {"seal": self.ctx.split_parts(True, n, P), "open": self.ctx.split_parts(False, n, P + 32)}
        text = self.layout == "neptun"
        for op, k in ks.items():
            if k > 1:
                tpl = "<true, false>" if op == "seal" else "<false, true>" if text else "<false, false>"
                self.kernels[op] = f"aead_strided_split_kernel{tpl} (K = {k}) + aead_strided_finish_kernel{tpl}"
        # the committed PMC summaries were profiled per size on the default slot shape
        default_shape = n == packets_for(args) and S == synth.round_up(P + 32, 128) and (
            self.layout == "neptun" or self.pad)
        base = "config2_neptun" if self.layout == "neptun" else "config2"
        self.profile_tag = (base if P == 1350 else f"{base}_p{P}") if default_shape else None

    def _seal_src(self):
        return (self.wire if self.layout == "neptun" else self.pt).data_ptr() + 16

    def prepare(self, stream):
        """--op open: seal the batch once, untimed, so every timed step opens it."""
        if self.op == "open":
            self.ctx.seal_strided(self.n, self.P, 0, self.counter_base, self._seal_src(), self.S,
                                  self.wire, self.S, self.st_seal, stream)

    def step(self, stream, evs=None):
        S, P, n = self.S, self.P, self.n
        if evs:
            evs[0].record(stream)
        if self.op != "open":
            self.ctx.seal_strided(n, P, 0, self.counter_base, self._seal_src(), S, self.wire, S,
                                  self.st_seal, stream)
        if evs:
            evs[1].record(stream)
        if self.op != "seal":
            self.ctx.open_strided(n, P + 32, 0, self.wire, S, self.back.data_ptr() + self.open_off, S,
                                  self.st_open, stream)
        if evs:
            evs[2].record(stream)

    def verify(self):
        import torch
        n, S, P, o = self.n, self.S, self.P, self.open_off
        if self.layout == "neptun":
            # the timed steps re-sealed the TUN buffers in place: one more step from
            # the original plaintext, then check that one
            self.wire.copy_(self.pt)
            self.back.zero_()
            self.ctx.seal_strided(n, P, 0, self.counter_base, self._seal_src(), S, self.wire, S,
                                  self.st_seal)
            self.ctx.open_strided(n, P + 32, 0, self.wire, S, self.back.data_ptr() + o, S, self.st_open)
            torch.cuda.synchronize()
        elif self.op == "seal":  # (the seal-only steps: open once, untimed, to check them)
            self.ctx.open_strided(n, P + 32, 0, self.wire, S, self.back.data_ptr() + o, S, self.st_open)
            torch.cuda.synchronize()
        ok = int((self.st_seal != 0).sum()) == 0 and int((self.st_open != 0).sum()) == 0
        return ok and torch.equal(self.back.view(n, S)[:, o:o + P], self.pt.view(n, S)[:, 16:16 + P])

    def outputs(self):
        """What a caller of the timed step holds after it: the sealed datagrams and the
        opened plaintexts of the sampled packets (one float32 per byte), and the two
        status arrays.  (--op seal / open: the buffer the op does not write is as the
        setup left it.)"""
        import numpy as np
        import torch
        n, S, P, o = self.n, self.S, self.P, self.open_off
        rows = dump_rows(np.full(n, P))
        sel = torch.from_numpy(rows).to(self.wire.device)
        return {"sample_rows": rows.astype(np.float64),
                "datagrams": to_host(self.wire.view(n, S)[sel][:, :P + 32].float()),
                "plaintexts": to_host(self.back.view(n, S)[sel][:, o:o + P].float()),
                **dump_statuses(rows, seal_status=self.st_seal, open_status=self.st_open)}

    def size_hist(self):
        return {self.P: self.n}

    def sample(self, k):
        """k (key, receiver_idx, counter, payload, datagram) tuples spread over the batch."""
        import numpy as np

        from tools import synth
        key = synth.keys(1)[0].tobytes()
        idx = np.unique(np.linspace(0, self.n - 1, min(k, self.n)).astype(np.int64))
        pt = self.pt.view(self.n, self.S)[idx].cpu().numpy()
        wire = self.wire.view(self.n, self.S)[idx].cpu().numpy()
        return [(key, synth.RECEIVER_IDX, self.counter_base + int(i), pt[j, 16:16 + self.P].tobytes(),
                 wire[j, :self.P + 32].tobytes()) for j, i in enumerate(idx)]

    def describe(self, world):
        what = {"roundtrip": "seal then open", "seal": "seal only (the reference's AEAD bench shape)",
                "open": "open only (of a batch sealed before timing)"}[self.op]
        cfg = ('2' if world == 1 else '5') if self.P == 1350 and self.op == "roundtrip" else \
            f"{'2' if world == 1 else '5'} shape at {self.P} B"
        d = {"workload": f"BASELINE config {cfg}: {self.n} x {self.P} B "
                         f"packets per GPU, single session, {what}, device-resident",
             "op": self.op,
             "packets_per_gpu": self.n, "packet_bytes": self.P, "slot_stride": self.S,
             "global_packets": world * self.n, "parallelism": f"{world} shard(s), no collective",
             "layout": self.layout,
             "slot_padding": ("writable: outputs zero-filled to their 128-byte line end "
                              "(wg_gpu_ctx_set_slot_padding)") if self.pad else "untouched"}
        if self.layout == "neptun":
            d["layout_note"] = ("NepTUN's buffers: seal in place (plaintext at slot+16 overwritten by "
                                "the datagram at slot+0, device/mod.rs:1297-1337), open into fresh "
                                "slots at offset 0 (device/mod.rs:1140-1148)")
        return d

    def close(self):
        self.ctx.close()


class DescWorkload:
    """Config 3 (mixed MTU, device-side length scheduling) and 4 (4096 peers)."""

    def __init__(self, args, dev, rank, world):
        import numpy as np

        import neptun_amd
        from tools import synth, workloads
        self.cfg = args.config
        if self.cfg == 3:
            sizes = tuple(int(x) for x in args.mixed_sizes.split(","))
            self.b = workloads.config3(args.per_size, dev, seed=synth.SEED + rank, sizes=sizes)
            nkeys = 1
        else:
            self.b = workloads.config4(args.peers, args.per_peer, args.size, dev,
                                       seed=synth.SEED + rank)
            nkeys = args.peers
        self.ctx = neptun_amd.GpuContext(dev.index, key_slots=nkeys)
        keys = synth.keys(nkeys)
        idx = np.full(nkeys, synth.RECEIVER_IDX, np.uint32) + np.arange(nkeys, dtype=np.uint32)
        self.ctx.set_keys(0, keys, idx)
        self.keys, self.key_index = keys, idx
        b = self.b
        self.packets = b.n
        P = b.sizes.astype(np.int64)
        self.payload_bytes = int(P.sum())
        key_bytes = 32 * b.n if self.cfg == 4 else 0  # per-lane key reads
        self.launch_bytes = {"seal": int((2 * P + 32).sum()) + key_bytes,
                             "open": int((2 * P + 32).sum()) + key_bytes}
        # config 3 runs the plan's ordered launches; config 4's unordered ones go to
        # the affine-capable kernel (wg_gpu.cpp, WG_DESC_AFFINE)
        # (config 3's context has one key slot: the SGPR-key form)
        k = "aead_desc_sync_key1_kernel" if self.cfg == 3 else "aead_desc_affine_kernel"
        self.kernels = {"seal": f"{k}<true>", "open": f"{k}<false>"}
        default_shape = (args.per_size == 1 << 18 and args.mixed_sizes == "64,256,576,1350,8900") \
            if self.cfg == 3 else (
            args.peers == 4096 and args.per_peer == 4096 and args.size == 1350)
        self.profile_tag = f"config{self.cfg}" if default_shape else None

    def step(self, stream, evs=None):
        b, ctx = self.b, self.ctx
        if evs:
            evs[0].record(stream)
        if self.cfg == 3:  # scheduling pass is part of the timed work
            ctx.plan_batch(True, b.d_seal, b.n, b.order, b.scratch, stream)
            ctx.seal_batch_ordered(b.d_seal, b.order, b.n, b.pt, b.wire, b.st_seal, stream)
        else:
            ctx.seal_batch(b.d_seal, b.n, b.pt, b.wire, b.st_seal, stream)
        if evs:
            evs[1].record(stream)
        if self.cfg == 3:  # open rounds = seal rounds (W = P + 32): same order
            ctx.open_batch_ordered(b.d_open, b.order, b.n, b.wire, b.out, b.st_open, stream)
        else:
            ctx.open_batch(b.d_open, b.n, b.wire, b.out, b.st_open, stream)
        if evs:
            evs[2].record(stream)

    def verify(self):
        b = self.b
        ok = int((b.st_seal != 0).sum()) == 0 and int((b.st_open != 0).sum()) == 0
        return ok and b.round_trip_equal()

    def outputs(self):
        """As StridedWorkload.outputs; the sampled packets differ in size, so their
        datagrams (and plaintexts) are concatenated in `sample_rows` order."""
        import numpy as np
        import torch
        b = self.b
        rows = dump_rows(b.sizes)
        dev = b.wire.device

        def gather(buf, starts, lens):
            first = np.repeat(starts - np.concatenate(([0], np.cumsum(lens)[:-1])), lens)
            idx = first + np.arange(int(lens.sum()), dtype=np.int64)
            return to_host(buf[torch.from_numpy(idx).to(dev)].float())

        P = b.sizes[rows].astype(np.int64)
        return {"sample_rows": rows.astype(np.float64),
                "datagrams": gather(b.wire, b.offs[rows], P + 32),
                "plaintexts": gather(b.out, b.offs[rows] + 16, P),
                **dump_statuses(rows, seal_status=b.st_seal, open_status=b.st_open)}

    def sample(self, k):
        return self.b.sample(k, self.keys, self.key_index)

    def size_hist(self):
        import numpy as np
        u, c = np.unique(self.b.sizes, return_counts=True)
        return {int(a): int(b) for a, b in zip(u, c)}

    def describe(self, world):
        import numpy as np
        b = self.b
        if self.cfg == 3:
            k = len(np.unique(b.sizes))
            w = (f"BASELINE config 3: mixed MTU {{{','.join(str(int(x)) for x in np.unique(b.sizes))}}} x "
                 f"{b.n // k} each, seeded interleave, single session, device-side length scheduling included")
        else:
            w = (f"BASELINE config 4: {b.n} x {int(b.sizes[0])} B packets over "
                 f"{self.ctx.key_slots} peers (per-lane key lookup from HBM)")
        return {"workload": w, "packets_per_gpu": b.n, "payload_bytes_per_gpu": self.payload_bytes,
                "global_packets": world * b.n, "parallelism": f"{world} shard(s), no collective"}

    def close(self):
        self.ctx.close()


def packets_for(args) -> int:
    """config 2 packets per GPU: --packets, else 1M x 1350 B worth of payload at --size."""
    if args.packets:
        return args.packets
    if args.size == 1350:
        return 1 << 20
    return max(512, (((1 << 20) * 1350 // max(args.size, 1)) // 512) * 512)


def make_workload(args, dev, rank, world):
    return StridedWorkload(args, dev, rank, world) if args.config == 2 else DescWorkload(
        args, dev, rank, world)


# ---------------------------------------------------------------------------
def host_cpus() -> dict:
    """The host's CPU model, its physical core count and the CPUs this process
    may run on (the GPU box grants each job a share of the machine)."""
    model, phys = "unknown", set()
    try:
        cur = {}
        with open("/proc/cpuinfo") as f:
            for line in f:
                if ":" in line:
                    k, v = (x.strip() for x in line.split(":", 1))
                    cur[k] = v
                    if k == "model name":
                        model = v
                elif cur:
                    phys.add((cur.get("physical id", "0"), cur.get("core id", cur.get("processor"))))
                    cur = {}
        if cur:
            phys.add((cur.get("physical id", "0"), cur.get("core id", cur.get("processor"))))
    except OSError:
        pass
    allowed = len(os.sched_getaffinity(0))
    return {"model": model, "physical_cores": len(phys) or (os.cpu_count() or 1),
            "logical_cpus": os.cpu_count() or 1, "allowed_cpus": allowed}


def smi_index(local: int) -> int:
    """amd-smi's index of this rank's GPU: HIP device `local` after any
    *_VISIBLE_DEVICES remapping (one process per GPU, torchrun's LOCAL_RANK)."""
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v:
            ids = [x.strip() for x in v.split(",") if x.strip()]
            if local < len(ids) and ids[local].isdigit():
                return int(ids[local])
    return local


class PowerSampler:
    """Socket power / gfx clock / PPT state of one GPU (`amd-smi metric -g`, read-only)
    sampled on a host thread while the supplementary sustained steps run: the
    kernels are power-bound, so the line says at what power and
    clock its sustained rate was reached.  Never fatal: no amd-smi -> an error note."""

    def __init__(self, period: float = 0.05, gpu: int = 0):
        import threading
        self.period, self.gpu, self.samples, self.error = period, gpu, [], None
        self._stop = threading.Event()
        self._thread = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        from tools import power_probe
        while not self._stop.is_set():
            s = power_probe.sample(self.gpu)
            if "err" in s:
                self.error = str(s["err"])[:120]
                return
            self.samples.append({"t": time.time(), "m": s})
            self._stop.wait(self.period)

    def start(self):
        self._thread.start()

    def stop(self) -> dict:
        from tools import power_probe
        self._stop.set()
        self._thread.join(timeout=30)
        if self.error and not self.samples:
            return {"error": self.error}
        return dict(power_probe.summarize(self.samples), amd_smi_gpu=self.gpu,
                    source="amd-smi metric during the sustained steps")


# the package power limit of MI355X (amd-smi reports PPT 1400 W on the boxes);
# a line is labelled power-limited only when its mean socket power reaches this
PPT_LIMITED_W = 1390.0


def power_limiter(pw: dict) -> str | None:
    """The roofline.limiter label: 'package power' only when the sustained steps
    drew the PPT limit (mean socket power >= PPT_LIMITED_W with PPT flagged),
    else None -- a PPT flag at lower mean power does not make the time
    power-set (config 4 at 1308-1328 W)."""
    if "ACTIVE" in pw.get("ppt_violation", []) and pw.get("socket_power_W", 0) >= PPT_LIMITED_W:
        # what holds the kernels below the HBM roofline
        return (f"package power: {pw['socket_power_W']} W with the PPT limit active at "
                f"{pw['gfx_clock_MHz']} MHz during the sustained steps; time per launch = energy "
                "per launch / power budget")
    return None


def cpu_baseline(threads: int, cpus: dict, curve=(), size: int = 1350, op: str = "roundtrip") -> dict:
    """Config 1 on the host cores: oracle/build/cpu_baseline (NepTUN framing over
    OpenSSL EVP, the stand-in for ring's asm; see oracle/cpu_baseline.c), one
    session and 64 Ki x 1350 B packets per worker thread like packet_workers.rs:113-131
    (num_cpus::get_physical() workers), each worker pinned to its own physical core
    with its buffers built on that core.  Measured at `threads` (this job's CPU share)
    and at each count of `curve` below it, so the per-core scaling behind the all-core
    figure is measured, not assumed."""
    exe = os.path.join(ROOT, "oracle", "build", "cpu_baseline")
    if not os.path.exists(exe):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)

    # config 1: 64 Ki x 1350 B per worker; at other sizes the same payload bytes per worker
    per_thread = 65536 if size == 1350 else max(1024, 65536 * 1350 // max(size, 1))
    # which figure is the baseline: the round trip (median wall), or the op run alone
    key = {"roundtrip": "gbps", "seal": "seal_gbps_best", "open": "open_gbps_best"}[op]

    def run(t, reps):
        out = subprocess.run([exe, "--impl", "openssl", "--threads", str(t), "--packets-per-thread",
                              str(per_thread), "--size", str(size), "--reps", str(reps), "--pin"],
                             capture_output=True, text=True, timeout=300)
        if out.returncode:
            raise RuntimeError(out.stderr)
        r = json.loads(out.stdout)
        r["gbps_op"] = r[key]
        return r

    one = run(1, 11)
    pts = {1: one["gbps_op"]}
    for t in sorted({int(c) for c in curve if 1 < int(c) < threads}):
        pts[t] = run(t, 9)["gbps_op"]
    many = run(threads, 9)
    pts[threads] = many["gbps_op"]
    eff = {t: g / t / one["gbps_op"] for t, g in pts.items()}
    # the all-core figure scales the per-core rate of the largest measured count
    # that still scaled (>= 0.8 of one core's rate per core): past it the job's
    # share of a machine other jobs also load is what gets measured
    t_ok = max(t for t, e in eff.items() if e >= 0.8)
    all_cores = threads >= cpus["physical_cores"]  # (a share that covers every core: measured)
    # the baseline is the best measured thread count (on a shared grant more threads can
    # measure less than fewer); the share's own point stays beside it
    t_best = max(pts, key=lambda t: pts[t])
    out = {
        "value": round(pts[t_best], 3),
        "unit": "Gbit/s",
        "cores": t_best,
        "value_at_share": round(many["gbps_op"], 3),
        "threads_at_share": threads,
        "kind": "port",
        "cpu_model": cpus["model"],
        "physical_cores": cpus["physical_cores"],
        "allowed_cpus": cpus["allowed_cpus"],
        "sample": (f"config 1 per worker: {per_thread} x {size} B encap+decap per thread ("
                   f"{ {'roundtrip': 'round-trip wall time', 'seal': 'best seal time', 'open': 'best open time'}[op] }"
                   f" is the figure), one session "
                   f"per thread, NepTUN framing (session.rs:205-302) over OpenSSL 3 EVP_chacha20_poly1305 "
                   f"(stand-in for ring 0.17 asm; the Rust reference cannot be built here), each thread "
                   f"pinned to its own physical core, median of 9 reps; value = the best measured thread "
                   f"count ({t_best}) of {sorted(pts)} up to this job's CPU share of {threads} "
                   f"({cpus['allowed_cpus']} CPUs in the affinity mask, {cpus['logical_cpus']} "
                   f"logical / {cpus['physical_cores']} physical cores on the machine, {cpus['model']}); "
                   f"1 thread: {one['gbps_op']:.3f} Gbit/s, {threads} threads: {many['gbps_op']:.3f} Gbit/s"),
        "one_core_gbps": round(one["gbps_op"], 3),
        "size": size, "op": op,
        "seal_gbps": round(many["seal_gbps_best"], 3), "open_gbps": round(many["open_gbps_best"], 3),
        "threads_gbps": {str(k): round(v, 3) for k, v in sorted(pts.items())},
        "scaling_efficiency": {str(k): round(v, 3) for k, v in sorted(eff.items())},
        "scaling_efficiency_at_share": round(eff[threads], 3),
        # the GPU box grants one job `threads` CPUs (its share: cgroup cpu.max) of a
        # machine whose other cores run other jobs, so the all-core figure is an
        # extrapolation from measured per-core rates -- labelled, not measured
        "all_physical_cores_extrapolated_gbps": round(pts[t_ok] / t_ok * cpus["physical_cores"], 1),
        # (the best per-core rate of any measured count: a noisy one-thread rep can sit
        # below the multi-thread per-core rates, and a bound must cover the estimate)
        "all_physical_cores_upper_bound_gbps": round(max(v / k for k, v in pts.items()) * cpus["physical_cores"], 1),
        "all_physical_cores_note": (f"per-core rate at {t_ok} pinned threads (the largest measured count "
                                    f"at >= 0.8 of one core's per-core rate) x physical cores; upper bound "
                                    f"= the best per-core rate of any measured count x physical cores.  Not "
                                    f"run on all cores: the GPU box grants one job a {threads}-CPU share of "
                                    f"the machine"),
    }
    if all_cores:
        out["all_physical_cores_gbps"] = out["value_at_share"]
        out["all_physical_cores_note"] = f"measured: the {threads} threads cover every physical core"
        del out["all_physical_cores_extrapolated_gbps"]
    return out


def evp_check(wl, k: int) -> dict:
    """Compare k sealed datagrams of the timed batch with OpenSSL EVP (tools/evp_check.py)."""
    if k <= 0 or not hasattr(wl, "sample"):
        return {"checked": 0}
    try:
        from tools.evp_check import Evp
        evp = Evp()
    except OSError as e:  # libcrypto missing: say so, never pass silently
        return {"checked": 0, "error": f"libcrypto unavailable: {e}"[:120]}
    bad = 0
    smp = wl.sample(k)
    for key, ridx, ctr, pt, wire in smp:
        bad += evp.seal_datagram(key, ridx, ctr, pt) != wire
    return {"checked": len(smp), "mismatches": bad}


def load_pmc(kind: str, kernel: str, tag: str | None) -> dict | None:
    """Committed rocprofv3 PMC summary of one bench kernel for this workload:
    kind "traffic" (tools/pmc_traffic.py, HBM bytes per launch) or "valu"
    (tools/pmc_valu.py, clock + VALU instructions per wave).  None when the
    workload is not the shape those summaries were profiled on."""
    if tag is None:
        return None
    path = os.path.join(ROOT, "profiles", f"pmc_{kind}_{tag}.json")
    if not os.path.exists(path):
        return None
    with open(path) as f:
        d = json.load(f)
    k = d.get("kernels", {}).get(kernel)
    if not k:
        return None
    return dict(k, source=os.path.relpath(path, ROOT), how=d.get("source", ""))


def compute_roofline(wl, kernel: str, kernel_ms: float, live_clock_ghz: float | None,
                     sustained_ms: float | None = None) -> dict | None:
    """VALU-issue floor of the launch (tools/compute_roofline.py), priced at the
    live gfx clock (amd-smi during this run's sustained steps) against the live
    kernel time; the PMC run's own clock and time only as frac_in_profiled_run."""
    from tools import compute_roofline as cr
    if not hasattr(wl, "size_hist"):
        return None
    keyed = getattr(wl, "cfg", 2) == 4  # per-lane keys: no SALU columns, no shared diagonal
    fl = cr.launch_floor(wl.size_hist(), live_clock_ghz, per_lane_keys=keyed)
    out = {"bound": "valu-issue", "model": "tools/compute_roofline.py", **fl}
    if live_clock_ghz:
        out["clock_GHz_live"] = round(live_clock_ghz, 4)
        out["clock_source"] = "amd-smi gfx clock, mean over the sustained steps of this run"
        out["frac"] = round(fl["floor_ms_at_clock"] / kernel_ms, 4)
        if sustained_ms:
            out["frac_sustained"] = round(fl["floor_ms_at_clock"] / sustained_ms, 4)
    pmc = load_pmc("valu", kernel, getattr(wl, "profile_tag", "config2"))
    if pmc:
        out.update({
            "clock_GHz_profiled": pmc["clock_GHz"],
            "frac_in_profiled_run": round(
                cr.launch_floor(wl.size_hist(), pmc["clock_GHz"], per_lane_keys=keyed)["floor_ms_at_clock"]
                / pmc["ms"], 4),
            "valu_instr_per_64_packets_measured": round(
                pmc["valu_per_wave"] * pmc.get("waves", 0) * 64 / wl.packets, 1),
            "pmc_source": pmc["source"],
        })
    return out


def mean(xs):
    return sum(xs) / len(xs) if xs else 0.0


def run(args, factory=None, device_fn=None, device_count=None):
    """Bench body.  `factory`/`device_fn`/`device_count` are injection points for
    the CPU tests of the multi-rank path (tests/test_bench_dist.py); production
    uses HIP."""
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        # a launcher's world and the flag disagree: publishing either count would lie
        if rank == 0:
            print(json.dumps({"error": f"--gpus {args.gpus} but WORLD_SIZE={world}: the rank count "
                                       "must equal --gpus", "n_gpus": world, "gpus_flag": args.gpus}),
                  flush=True)
        return 2
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    visible = torch.cuda.device_count() if device_count is None else device_count
    if world > visible:
        # one process per GPU: an N-GPU line from ranks sharing devices would be
        # published as scaling it is not -- refuse instead
        if rank == 0:
            print(json.dumps({"error": f"{world} ranks but {visible} visible GPU(s): one rank per "
                                       "GPU is required, refusing to share devices",
                              "n_gpus": world, "visible_gpus": visible}), flush=True)
        if world > 1:
            dist.destroy_process_group()
        return 2
    if device_fn is None:
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
        stream = torch.cuda.current_stream(dev)
        sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
        new_event = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    else:
        dev, stream, sync, new_event = device_fn(local)

    wl = (factory or make_workload)(args, dev, rank, world)
    if hasattr(wl, "prepare"):
        wl.prepare(stream)
    for _ in range(args.warmup):
        wl.step(stream)
    sync()

    events = [[new_event() for _ in range(3)] for _ in range(args.steps)]
    if world > 1:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for k in range(args.steps):
        wl.step(stream, events[k])
    sync()
    elapsed = time.perf_counter() - t0
    my_elapsed = elapsed
    totals = torch.tensor([wl.payload_bytes, wl.packets], dtype=torch.float64)
    if world > 1:
        dist.barrier()
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        dist.all_reduce(totals, op=dist.ReduceOp.SUM)

    seal_ms = [e[0].elapsed_time(e[1]) for e in events]
    open_ms = [e[1].elapsed_time(e[2]) for e in events]
    if os.environ.get("BENCH_STEP_TRACE"):  # diagnostics: per-step kernel times on stderr
        print(json.dumps({"seal_ms": [round(x, 4) for x in seal_ms],
                          "open_ms": [round(x, 4) for x in open_ms]}), file=sys.stderr, flush=True)

    # what the last timed step left, before anything below runs the kernels again
    dumped = dump_outputs(wl, args.dump_outputs, rank, world) if args.dump_outputs else None

    # --full: correctness of what was timed: statuses + round-trip identity (whole
    # batch) + a sample of sealed datagrams byte for byte against OpenSSL EVP
    ok, evp = True, None
    if args.full:
        ok = bool(wl.verify())
        evp = evp_check(wl, args.evp_sample)
        ok = ok and evp.get("mismatches", 0) == 0
        if world > 1:
            f = torch.tensor([0 if ok else 1], dtype=torch.int64)
            dist.all_reduce(f, op=dist.ReduceOp.MAX)
            ok = int(f.item()) == 0
    sustained = None
    if args.full and ok and args.sustain_seconds > 0:
        # the kernels run at the package power limit (profiles/r02_power.json);
        # over the first tens of ms the clock is still settling, so the K-step
        # line above and a seconds-long run can differ by a few %.  Every rank
        # runs it at once (its own GPU's power and clock sampled), so an N-GPU
        # line says what each package did while all of them were loaded.
        per = max(my_elapsed / args.steps, 1e-4)
        k2 = max(1, int(args.sustain_seconds / per))
        if world > 1:  # one count for all ranks: they start and end together
            kt = torch.tensor([k2], dtype=torch.int64)
            dist.all_reduce(kt, op=dist.ReduceOp.MIN)
            k2 = int(kt.item())
        evs = [[new_event() for _ in range(3)] for _ in range(k2)]
        sampler = PowerSampler(gpu=smi_index(local)) if device_fn is None else None
        sync()
        if world > 1:
            dist.barrier()
        if sampler:
            sampler.start()  # samples while the steps run (idle samples are filtered out)
        for k in range(k2):
            wl.step(stream, evs[k])
        sync()
        ms = evs[0][0].elapsed_time(evs[-1][2])
        sustained = {"steps": k2, "seconds": round(ms * 1e-3, 3),
                     "gbps": round(wl.payload_bytes * 8 * k2 / (ms * 1e-3) / 1e9, 2),
                     "ms_per_step": round(ms / k2, 4),
                     "kernel_ms": {"seal": round(mean([e[0].elapsed_time(e[1]) for e in evs]), 4),
                                   "open": round(mean([e[1].elapsed_time(e[2]) for e in evs]), 4)},
                     "note": "supplementary: steps run after the timed region and its "
                             "verification; not the headline value"}
        if sampler:
            sustained["power"] = sampler.stop()
            pw_e = sustained["power"].get("socket_power_from_energy_W")
            if pw_e:  # package energy per packet round trip (seal + open), at the sustained rate
                sustained["power"]["energy_uJ_per_packet_roundtrip"] = round(
                    pw_e * (ms / k2) * 1e-3 / wl.packets * 1e6, 4)
    avg = {"seal": mean(seal_ms), "open": mean(open_ms)}
    mine = {"rank": rank, "local_rank": local, "elapsed_s": round(my_elapsed, 6),
            "kernel_ms": {k: round(v, 4) for k, v in avg.items()},
            "packets": wl.packets, "payload_bytes": wl.payload_bytes}
    if sustained:
        mine["sustained_gbps"] = sustained["gbps"]
        mine["sustained_kernel_ms"] = sustained["kernel_ms"]
        if "power" in sustained:
            mine["power"] = sustained["power"]
    per_rank = [mine]
    if world > 1:
        per_rank = [None] * world
        dist.all_gather_object(per_rank, mine)
    line = None
    if not ok:
        line = {"error": "verification failed (statuses, round trip or EVP sample)", "rank": rank,
                "evp_sample": evp}
    elif rank == 0:
        total_payload, total_pkts = float(totals[0]), float(totals[1])
        gbps = total_payload * 8 * args.steps / elapsed / 1e9
        op = getattr(wl, "op", "roundtrip")
        ran = ["seal", "open"] if op == "roundtrip" else [op]
        dom = max(ran, key=lambda k: avg[k])
        achieved = wl.launch_bytes[dom] / (avg[dom] * 1e-3) / 1e9
        tag = getattr(wl, "profile_tag", f"config{args.config}")  # (None: non-default shape)
        tr = load_pmc("traffic", wl.kernels[dom], tag)
        pw = (sustained or {}).get("power") or {}
        live_clock = pw["gfx_clock_MHz"] / 1e3 if pw.get("gfx_clock_MHz") else None
        if args.config != 2:
            metric = f"Gbit/s device-resident ChaCha20-Poly1305 seal+open, BASELINE config {args.config}"
        elif op == "roundtrip" and args.size == 1350:
            metric = METRIC
        else:
            metric = (f"Gbit/s device-resident ChaCha20-Poly1305 "
                      f"{ {'roundtrip': 'seal+open', 'seal': 'seal', 'open': 'open'}[op] }, {args.size}B pkts")
        live_clk = live_clock
        per_kernel = {}
        for k in ran:  # each launch against both rooflines
            kb = wl.launch_bytes[k] / (avg[k] * 1e-3) / 1e9
            cr_k = compute_roofline(wl, wl.kernels[k], avg[k], live_clk,
                                    ((sustained or {}).get("kernel_ms") or {}).get(k))
            per_kernel[k] = {"kernel": wl.kernels[k], "ms": round(avg[k], 4),
                             "gbps_payload": round(wl.payload_bytes * 8 / (avg[k] * 1e-3) / 1e9, 1),
                             "hbm_frac": round(kb / HBM_PEAK_GBS, 4),
                             "compute_frac": (cr_k or {}).get("frac"),
                             "floor_ms_at_live_clock": (cr_k or {}).get("floor_ms_at_clock")}
        line = {
            "metric": metric,
            "value": round(gbps, 2),
            "unit": "Gbit/s",
            "n_gpus": world,
            "visible_gpus": visible,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u32",
            "data": "synthetic (seeded payloads and keys; counters = lane index / per-peer rank)",
            "config": wl.describe(world),
            "roofline": {
                "bound": "hbm",
                "kernel": dom,
                "achieved": round(achieved, 1),
                "peak": HBM_PEAK_GBS,
                "unit": "GB/s",
                "frac": round(achieved / HBM_PEAK_GBS, 4),
                "traffic": tr["hbm_bytes_per_launch"] if tr else None,
                "traffic_over_algorithmic": round(tr["hbm_bytes_per_launch"] / wl.launch_bytes[dom], 4)
                if tr else None,
                "traffic_source": tr["source"] if tr else None,
                "algorithmic_bytes_per_launch": wl.launch_bytes[dom],
                # the bound that actually limits the kernel: VALU issue
                "compute": compute_roofline(wl, wl.kernels[dom], avg[dom], live_clock,
                                            ((sustained or {}).get("kernel_ms") or {}).get(dom)),
            },
            "kernel_ms": {k: round(avg[k], 4) for k in ran},
            **{f"{k}_gbps": per_kernel[k]["gbps_payload"] for k in ran},
            "per_kernel": per_kernel,
            "roundtrip_hbm_frac": round(sum(wl.launch_bytes[k] for k in ran) /
                                        (sum(avg[k] for k in ran) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "packets_per_step": int(total_pkts),
            "full": args.full,
        }
        if args.full:
            line.update({
                "verified": "all statuses Ok, open(seal(x)) == x over the whole batch, and "
                            f"{evp.get('checked', 0)} sealed datagrams spread over the batch equal "
                            "OpenSSL EVP_chacha20_poly1305 with NepTUN framing",
                "evp_sample": evp,
                "sustained": sustained,
            })
        if dumped:
            line["dumped_outputs"] = dumped
        if world > 1:
            line["per_rank"] = per_rank
        lim = power_limiter(pw)
        if lim:
            line["roofline"]["limiter"] = lim
        if args.full and world == 1 and not args.no_cpu_baseline and args.config == 2:
            # (at --size P and --op: the CPU path at the same size, the same operation)
            cpus = host_cpus()
            # one thread per physical core this job may use: the GPU box grants a
            # job a CPU share (OMP_NUM_THREADS there) of a larger machine
            share = int(os.environ.get("OMP_NUM_THREADS") or cpus["allowed_cpus"])
            threads = args.cpu_threads or max(1, min(cpus["allowed_cpus"], cpus["physical_cores"], share))
            curve = [int(x) for x in args.cpu_curve.split(",") if x.strip()] if args.cpu_curve else []
            try:
                line["cpu_baseline"] = cpu_baseline(threads, cpus, curve, size=args.size, op=op)
            except Exception as e:  # reported, never fatal to the GPU number
                line["cpu_baseline"] = {"error": str(e)[:200]}
    if line is not None:
        print(json.dumps(line), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    wl.close()
    return 0 if ok else 1


def _free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def launch_local(n: int, argv: list[str]) -> int:
    """`bench.py --gpus N` without a launcher: start N rank processes of this same
    script, one per GPU (the reference's one worker per core, packet_workers.rs:113-131,
    becomes one rank per GPU), with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set the
    way torchrun sets them.  Nothing here touches the GPU (children are started, never
    exec'd into); rank 0 prints the line.  If a rank dies, the others are stopped
    instead of waiting at a barrier.  Returns the worst exit code."""
    env0 = dict(os.environ, WORLD_SIZE=str(n), MASTER_ADDR="127.0.0.1",
                MASTER_PORT=str(_free_port()), LOCAL_WORLD_SIZE=str(n))
    procs = []
    for r in range(n):
        env = dict(env0, RANK=str(r), LOCAL_RANK=str(r))
        procs.append(subprocess.Popen([sys.executable, "-u", os.path.abspath(__file__), *argv], env=env))
    rcs: dict[int, int] = {}
    failed_at = None
    while len(rcs) < n:
        for r, p in enumerate(procs):
            if r not in rcs and p.poll() is not None:
                rcs[r] = p.returncode
                if p.returncode != 0 and failed_at is None:
                    failed_at = time.time()
        if failed_at is not None and time.time() - failed_at > 30:
            for r, p in enumerate(procs):  # the exact children started above
                if r not in rcs:
                    p.kill()
        time.sleep(0.05)
    bad = [rc for rc in rcs.values() if rc != 0]
    return max(bad, key=abs) if bad else 0


def main():
    args = parse()
    ws = os.environ.get("WORLD_SIZE")
    if ws is None and args.gpus > 1:
        sys.exit(launch_local(args.gpus, sys.argv[1:]))
    hook = os.environ.get("BENCH_FAKE_DEVICE")
    if hook:  # test-only: the CPU stand-in of tests/bench_fake.py (never on a GPU run)
        import importlib
        m = importlib.import_module(hook)
        sys.exit(run(args, factory=m.FakeWorkload, device_fn=m.cpu_device,
                     device_count=int(os.environ.get("BENCH_FAKE_GPUS", args.gpus))))
    sys.exit(run(args))


if __name__ == "__main__":
    main()
