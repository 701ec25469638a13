"""Lookups per second of the AllowedIPs kernels (wg_gpu_allowed_route_batch /
wg_gpu_allowed_filter_batch) on a device-resident batch, with wg_gpu_route_batch's
route_kernel on the same batch for scale.

    python tools/allowed_bench.py [--packets 1048576] [--len 1350] [--values 4096] [--v6 0.25]

1,048,576 packets of 1350 bytes in 1408-byte slots; a table of 4096 values with two
networks each (an IPv4 /24 and an IPv6 /48); every packet's destination and source lie
in a network of a random value.  Each kernel: 5 warm-up launches, then the median of 20
launches timed with device events.  The algorithmic bytes per packet are the 32-byte
descriptor, one 128-byte line of the header and what the kernel stores (route: value
and key slot, 8 bytes; filter: the 4-byte status read and 1 byte written); their rate is
printed as a share of the HBM peak (8.0 TB/s).  Prints one JSON line.  Not a test and
not part of bench.py.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12  # bytes/s


def timed(torch, fn, warmup=5, reps=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms) * 1e-3, min(ms) * 1e-3, max(ms) * 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--len", type=int, default=1350)
    ap.add_argument("--values", type=int, default=4096)
    ap.add_argument("--v6", type=float, default=0.25, help="share of IPv6 packets")
    args = ap.parse_args()
    import torch

    from neptun_amd import AllowedIps, GpuContext
    from neptun_amd.gpu import DESC_DTYPE

    n, P, V = args.packets, args.len, args.values
    S = (P + 32 + 127) // 128 * 128
    rng = np.random.default_rng(1)

    table = AllowedIps()
    for v in range(V):
        table.insert(bytes([10, v >> 8, v & 255, 0]), 24, v)
        table.insert(bytes([0xfd, 0, 0, 0, v >> 8, v & 255]) + bytes(10), 48, v)

    # headers: destination and source inside a network of the packet's value
    val = rng.integers(0, V, n, dtype=np.uint32)
    is6 = rng.random(n) < args.v6
    hdr = rng.integers(0, 256, (n, 40), dtype=np.uint8)
    hdr[:, 0] = np.where(is6, 0x60, 0x45)
    v4 = np.stack([np.full(n, 10, np.uint8), (val >> 8).astype(np.uint8), (val & 255).astype(np.uint8),
                   rng.integers(0, 256, n, dtype=np.uint8)], 1)
    m4 = ~is6
    hdr[m4, 12:16] = v4[m4]
    hdr[m4, 16:20] = v4[m4]
    v6 = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    v6[:, 0], v6[:, 1:4] = 0xfd, 0
    v6[:, 4], v6[:, 5] = (val >> 8).astype(np.uint8), (val & 255).astype(np.uint8)
    hdr[is6, 8:24] = v6[is6]
    hdr[is6, 24:40] = v6[is6]

    if not torch.cuda.is_available():
        raise SystemExit("allowed_bench needs a GPU")
    buf = torch.zeros(n * S, dtype=torch.uint8, device="cuda")
    buf.view(n, S)[:, :40] = torch.from_numpy(hdr).cuda()
    descs = np.zeros(n, DESC_DTYPE)
    descs["src_off"] = np.arange(n, dtype=np.uint64) * S
    descs["dst_off"] = descs["src_off"]
    descs["len"] = P
    d_route = torch.from_numpy(descs.view(np.uint8).reshape(-1).copy()).cuda()
    descs["len"] = P + 32          # the filter sees an opened datagram: plaintext = len - 32
    descs["key_slot"] = val * 16   # >> 4: the value
    d_filter = torch.from_numpy(descs.view(np.uint8).reshape(-1).copy()).cuda()
    d_val = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")

    out = {"packets": n, "len": P, "slot": S, "values": V, "networks": len(table), "v6_share": args.v6}
    with GpuContext(0, key_slots=V * 16) as ctx:
        ctx.allowed_set(table)
        t_route = timed(torch, lambda: ctx.allowed_route_batch(d_route, n, buf, d_val, True))
        got = d_val.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, val), "routed values differ from the packets' values"
        t_filter = timed(torch, lambda: ctx.allowed_filter_batch(d_filter, n, buf, d_st, d_ok, None, 4))
        assert int(d_ok.sum()) == n, "every source lies in its value's network"
        # route_kernel on the same batch: DATA headers whose receiver index is in the table
        ridx = (val.astype(np.uint64) * 2654435761 % (1 << 32)).astype(np.uint32)
        uniq = np.unique(ridx)
        ctx.route_set(uniq, np.arange(len(uniq), dtype=np.uint32) % (V * 16))
        head = np.zeros((n, 8), np.uint8)
        head[:, 0] = 4
        head[:, 4:8] = ridx.view(np.uint8).reshape(n, 4)
        buf.view(n, S)[:, :8] = torch.from_numpy(head).cuda()
        t_ridx = timed(torch, lambda: ctx.route_batch(d_filter, n, buf))
        ctx.allowed_set(None)
    for name, t, nbytes in (("allowed_route_batch", t_route, 32 + 128 + 8),
                            ("allowed_filter_batch", t_filter, 32 + 128 + 4 + 1),
                            ("route_batch", t_ridx, 32 + 128 + 4)):
        med, lo, hi = t
        out[name] = {"median_us": round(med * 1e6, 2), "min_us": round(lo * 1e6, 2), "max_us": round(hi * 1e6, 2),
                     "lookups_per_s": round(n / med), "ns_per_packet": round(med / n * 1e9, 4),
                     "algorithmic_bytes_per_packet": nbytes,
                     "algorithmic_bytes_per_s": round(n * nbytes / med),
                     "share_of_hbm_peak": round(n * nbytes / med / HBM_PEAK, 4)}
    for name in ("allowed_route_batch", "allowed_filter_batch"):
        out[name]["times_route_batch"] = round(out[name]["median_us"] / out["route_batch"]["median_us"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
