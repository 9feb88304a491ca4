#!/usr/bin/env python3
"""Work lists of k_schur_items for the two bench scenes -> tools/l2sim/l2sim (an offline LRU model of an XCD's L2): the items cut
into contiguous stretches (what item_beg / item_end say) against the shipped descriptors (blocks of >= 3 items interleaved) and
against interleaving blocks of 2 items as well, at 640 waves and 4 MiB.
usage: run.py [visibility ...] [--cams C --pts P] [--pace X ...]   (default: random nearest, 200 100000, pace 1.0)"""
import argparse, os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from sfm_amd import synth
from sfm_amd.structure import build_structure
ap = argparse.ArgumentParser()
ap.add_argument("visibility", nargs="*", default=["random", "nearest"])
ap.add_argument("--cams", type=int, default=200)
ap.add_argument("--pts", type=int, default=100000)
ap.add_argument("--pace", type=float, nargs="*", default=[1.0], help="speed of self-pair items relative to the others")
args = ap.parse_args()
here = os.path.dirname(os.path.abspath(__file__))
tmp = tempfile.mkdtemp(prefix="l2sim_")
exe = os.path.join(tmp, "l2sim")
subprocess.run(["gcc", "-O2", "-o", exe, os.path.join(here, "l2sim.c")], check=True)


def interleaved(st, n_min):
    """Descriptors with every block of >= n_min items interleaved (n_min = 3: what ships)."""
    n = np.repeat(np.diff(st.item_ptr), np.diff(st.item_ptr)).astype(np.int64)
    owner = np.repeat(np.arange(len(st.item_ptr) - 1), np.diff(st.item_ptr))
    i = np.arange(st.n_items) - st.item_ptr[owner]
    lo, hi = st.blk_ptr[owner].astype(np.int64), st.blk_ptr[owner + 1].astype(np.int64)
    il = n >= n_min
    return (np.where(il, lo + i, st.item_beg), np.where(il, n, 1), np.where(il, (hi - lo - i + n - 1) // n, st.item_end - st.item_beg))


for vis in args.visibility:
    sc = synth.make_scene(args.cams, args.pts, obs_per_point=10, seed=1004, noise_px=0.5, pt_sigma=0.02, cam_sigma=0.002, visibility=vis)
    st = build_structure(sc.cam_idx, sc.pt_idx, args.cams, args.pts)
    print(vis, "pairs", st.n_pairs, "items", st.n_items, "items per XCD group", np.diff(st.xcd_ptr).tolist(), flush=True)
    shipped = (st.item_first, st.item_stride, st.item_cnt)
    assert all(np.array_equal(a, b) for a, b in zip(shipped, interleaved(st, 3)))
    cuts = (("contiguous", (st.item_beg, np.ones_like(st.item_beg), st.item_end - st.item_beg)), ("interleave >= 3 (shipped)", shipped),
            ("interleave >= 2", interleaved(st, 2)))
    for name, desc in cuts:
        out = os.path.join(tmp, "work.bin")
        with open(out, "wb") as f:
            np.array([st.n_pairs, st.n_items, 2, 0], dtype=np.int64).tofile(f)
            for a in (st.pair_k, st.pair_k2) + tuple(desc) + (st.xcd_ptr, st.xcd_items):
                np.ascontiguousarray(a, dtype=np.int32).tofile(f)
        for pace in args.pace:
            print("  %-26s" % name, end=" ", flush=True)
            subprocess.run([exe, out, "640", "4", "8", str(pace)], check=True)
