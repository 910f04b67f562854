#!/usr/bin/env python3
"""GPU box: the update family of a Stage-I step -- per sub-network the mode-1 fmri_apply_batch launch and the
fmri_transpose_f16_batch launch behind it -- timed alone, against fmri_rmsprop_dev over the same parameter count (the
box's own rate for a pass of this kind: 20 bytes per parameter, no layout map).

The three sub-networks are built at a small batch (the update does not depend on it) and one step is run, so that the
device tables exist; the launches are then replayed from those tables.  Timing as bench.py's hbm_rows: 10 calls recorded
into a HIP graph, 20 replays.  Bytes by the accounting of the kernels' headers (csrc/layout.hip): 22 per parameter for
the update, 4 per element for the transposes.  That accounting takes one slab per tensor; ``mbytes_moved`` /
``gb_s_moved`` count what the table really asks for: 16 bytes of w / sq traffic, 2 of the fp16 copy where the row has
one, and 4 per slab read, 4 more per slab of a row whose slabs are handed back zeroed.  Replaying the update is
harmless: the gradient buffers come back zeroed or keep their values, the weights stay finite.

Prints one line per launch and one JSON line.

usage: tools/time_update_family.py [--batch 8] [--reps 20] [--inner 10]
"""
import argparse
import json
import os
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "thesis-fmri-reconstruction_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

APPLY_ENTRY = np.dtype([("gsrc", "<u8"), ("w", "<u8"), ("sq", "<u8"), ("grad", "<u8"), ("pk", "<u8"), ("sa", "<i8"),
                        ("sta", "<i8"), ("sb", "<i8"), ("slab_stride", "<i8"), ("n", "<i8"), ("A", "<i4"), ("TA", "<i4"),
                        ("B", "<i4"), ("Bp", "<i4"), ("run", "<i4"), ("ld", "<i4"), ("kpad", "<i4"), ("nslabs", "<i4"),
                        ("clear", "<i4"), ("kind", "<i4"), ("bt", "<i4"), ("tile_begin", "<i4"), ("scale", "<f4"),
                        ("vec", "<i4")])
TRANSPOSE_ENTRY = np.dtype([("src", "<u8"), ("dst", "<u8"), ("R", "<i4"), ("C", "<i4"), ("Rbuf", "<i4"), ("width", "<i4"),
                            ("lds", "<i4"), ("ldd", "<i4"), ("tile_begin", "<i4"), ("pad", "<i4")])


def timed(fn, reps, inner):
    """GPU microseconds per call: ``inner`` calls in a HIP graph, ``reps`` replays."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (reps * inner) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=10)
    a = ap.parse_args()
    from fmri_hip import lib, ops
    from fmri_hip.params import ArchConfig
    from fmri_hip.steps import Stage1Step
    L = lib.load()
    P = lib.ptr
    dev = torch.device("cuda:0")
    cfg = ArchConfig.px64()
    st = Stage1Step(cfg, dev)
    st.load_recipe(0, False)
    if hasattr(st, "gate_skip"):
        st.gate_skip = False
    rs = np.random.RandomState(5)
    x = torch.from_numpy(rs.uniform(-1, 1, (a.batch, 3, 64, 64)).astype(np.float32)).to(dev)
    nz = torch.from_numpy(rs.standard_normal((2, a.batch, cfg.latent_dim)).astype(np.float32)).to(dev)
    st.step(x, nz[0], nz[1])
    torch.cuda.synchronize()
    assert APPLY_ENTRY.itemsize == L.fmri_apply_entry_bytes() and TRANSPOSE_ENTRY.itemsize == L.fmri_transpose_entry_bytes()

    opts = [v for v in vars(st).values() if hasattr(v, "s1") and hasattr(v, "lr_dev") and hasattr(v, "g")]
    rows, out = [], {"batch": a.batch, "reps": a.reps, "inner": a.inner, "launches": []}

    def report(name, us, nbytes, extra=None):
        r = dict(name=name, us=round(us, 2), mbytes=round(nbytes / 1e6, 2), gb_s=round(nbytes / us / 1e3, 1))
        r.update(extra or {})
        rows.append(r)
        out["launches"].append(r)

    for o in opts:
        q = ops.grad_queue(o.g)
        plans = [p for p in q.plans.values() if p["key"][-1] is True and p["n"]]
        if not plans:
            continue
        plan = max(plans, key=lambda p: p["tiles"])
        n = int(o.g.numel)
        name = next((k for k, v in vars(st).items() if getattr(v, "group", None) is o.g), "group") + f" ({n} parameters)"
        tab = plan["table"].cpu().numpy().view(APPLY_ENTRY)
        elems = np.where(tab["kind"] == 2, tab["n"], tab["A"].astype(np.int64) * tab["TA"] * tab["B"] * tab["run"])
        per = np.where(tab["kind"] == 2, 20, 16 + 2 * (tab["pk"] != 0) + 4 * tab["nslabs"] * (1 + (tab["clear"] != 0)))
        moved = float((elems * per).sum())
        nvec = int(elems[tab["vec"] != 0].sum())
        us = timed(lambda: lib.call("fmri_apply_batch", P(plan["table"]), plan["n"], plan["tiles"], 1, P(o.lr_dev), o.alpha,
                                    o.eps, 1.0, None, 0.0, None, 0), a.reps, a.inner)
        report("apply_batch mode 1: " + name, us, 22.0 * int(elems.sum()),
               dict(rows=int(plan["n"]), tiles=int(plan["tiles"]), elements=int(elems.sum()), elements_in_16_byte_rows=nvec,
                    mbytes_moved=round(moved / 1e6, 2), gb_s_moved=round(moved / us / 1e3, 1),
                    slabs_of_the_largest_row=int(tab["nslabs"][int(np.argmax(elems))])))
        for t in q.pack_tables.values():
            if t["t_n"]:
                tt = t["t_table"].cpu().numpy().view(TRANSPOSE_ENTRY)
                el = int((tt["R"].astype(np.int64) * tt["C"]).sum())
                us = timed(lambda: lib.call("fmri_transpose_f16_batch", P(t["t_table"]), t["t_n"], t["t_tiles"]), a.reps,
                           a.inner)
                report("transpose_f16_batch: " + name, us, 4.0 * el, dict(rows=int(t["t_n"]), tiles=int(t["t_tiles"]),
                                                                           elements=el))
                break
        p, g, sq = (torch.randn(n, device=dev) for _ in range(3))
        sq.abs_()
        us = timed(lambda: lib.call("fmri_rmsprop_dev", P(p), P(g), P(sq), n, P(o.lr_dev), 0.9, 1e-8, 1.0, None, 0.0, None),
                   a.reps, a.inner)
        report("rmsprop_dev yardstick: " + name, us, 20.0 * n)
        del p, g, sq
    for r in rows:
        print("%-62s %8.2f us %9.2f MB %8.1f GB/s" % (r["name"], r["us"], r["mbytes"], r["gb_s"])
              + (" | moved %9.2f MB %8.1f GB/s" % (r["mbytes_moved"], r["gb_s_moved"]) if "mbytes_moved" in r else ""), flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
