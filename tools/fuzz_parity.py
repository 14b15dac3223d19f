#!/usr/bin/env python3
"""Random-shape parity sweep (GPU operator vs the oracle): frames, channel counts, degrees, batch counts and
input/output cloud sizes drawn at random.  Next to the whole-tensor errors it prints the row-wise ratios of tests/rowwise_error.py
(entry=ratio@slice) and holds both to the suite's bounds.  Prints the kernel forms every case takes (se3conv_forms) and ends with the forms
the run reached that no table of the suite runs (tests/test_form_coverage.py keeps that list empty for the shapes it sweeps).
usage: tools/fuzz_parity.py [n_cases] [seed]"""
import os, sys, random
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import se3conv3d_amd as amd
from oracle import se3conv_oracle as O
import test_gpu_parity as T
import form_coverage_table as FC
import rowwise_error as RW

n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
rng = random.Random(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
worst = 0.0
reached = {}


def note_forms(label, geom, c_in, c_out, prec):
    """the forms of the calls run_case_against_oracle makes (the autograd node's request) for this case"""
    shp = geom.shape(c_in, c_out, 32, prec)
    shape = (prec, shp.n_in, shp.n_out, shp.n_edges, shp.f_in, shp.f_out, shp.c_in, shp.c_out)
    names = sorted(set().union(*(FC.forms(shape, r) for r in FC.module_requests(shape))))
    for name in names:
        reached.setdefault(name, label)
    print("        forms: " + " ".join(names))


for i in range(n_cases):
    f_in, f_out = rng.choice([1, 2, 3, 4, 6]), rng.choice([1, 2, 3, 4, 6])
    c_in = rng.choice([1, 3, 8, 16, 24, 32, 48, 64, 80, 96, 128, 160, 192, 256, 320])
    c_out = rng.choice([5, 13, 32, 64, 96, 128, 192, 256])
    n_in = rng.choice([97, 200, 333, 500])
    n_out = rng.choice([None, None, 64, 150, 400])
    k_deg = rng.choice([2, 8, 16, 33, 50])
    batches = rng.choice([1, 2, 3])
    if n_out is None and f_in != f_out and rng.random() < 0.5:
        f_out = f_in
    c = T.random_case(100 + i, n_in, n_out, f_in, f_out, c_in, c_out, k_deg, batches)
    nb_ref, ends_ref, rho, nu = RW.graph_of(c)
    rowwise = RW.reference_and_scales(c, nb_ref, rho, nu)  # the fp64 reference and the scales, once per case
    oracle = (nb_ref, ends_ref, tuple(rowwise[0][k] for k in RW.KEYS))
    for prec in ("bf16x3", "fp32", "bf16x3_t16"):
        amd.set_precision(prec)
        errs, ratios, geom, nb_ref = T.run_case_rowwise_against_oracle(c, f_in, f_out, amd, oracle, rowwise)
        m = max(errs.values())
        rw = max(ratios[k] / RW.TOLERANCES[prec][k] for k in RW.ENTRIES) if ratios["zeros_exact"] else float("inf")
        worst = max(worst, m / T.TOLS[prec], rw)
        flag = "" if m < T.TOLS[prec] and rw < 1.0 else "   <-- FAIL"
        print(f"case {i:2d} {prec:6s} F {f_in}->{f_out} C {c_in:3d}->{c_out:3d} n {n_in}->{n_out} k~{k_deg:2d} b{batches}: "
              f"max rel err {m:.2e}  rowwise {RW.fmt(ratios)} (worst {rw:.2f} of its bound){flag}")
        note_forms(f"case {i} {prec}", geom, c_in, c_out, prec)
# larger clouds with narrow rows: >= 2048 output rows (strip GEMM), the grid search of the ball query, the two-stream
# range of backward; sizes the CPU oracle still finishes in seconds
for i in range(max(2, n_cases // 8)):
    f = rng.choice([1, 2])
    n_in = rng.choice([2600, 4500])
    c_in, c_out = rng.choice([(16, 32), (32, 32), (64, 64), (32, 64)])
    if n_in > 3000 and c_in * c_out > 1024:
        c_in = c_out = 32
    c = T.random_case(500 + i, n_in, rng.choice([None, None, 1200]), f, f, c_in, c_out, rng.choice([6, 9]), rng.choice([1, 2]))
    for prec in ("bf16x3", "fp32", "bf16x3_t16"):
        amd.set_precision(prec)
        errs, geom, _ = T.run_case_against_oracle(c, f, f, amd)
        m = max(errs.values())
        worst = max(worst, m / T.TOLS[prec])
        flag = "" if m < T.TOLS[prec] else "   <-- FAIL"
        print(f"large {i} {prec:6s} F {f} C {c_in:3d}->{c_out:3d} n {n_in}: max rel err {m:.2e}{flag}")
        note_forms(f"large {i} {prec}", geom, c_in, c_out, prec)
in_tables = FC.covered()
print("forms this run reached that no table of the suite runs: "
      + (", ".join(f"{n} ({w})" for n, w in sorted(reached.items()) if n not in in_tables) or "none"))
print(f"worst error / tolerance = {worst:.3f}")
sys.exit(0 if worst < 1.0 else 1)
