"""The array forms of the restatements (local_ref.spill_fast / LocalMap, global_ref.hash_fast / pair_step_fast) against their dict
forms, which stay the definition: identical bytes, counts and order on random and adversarial inputs -- duplicates, NaN / inf keys,
every record in one key, every record its own key, float keys shared by neighbouring cells far from the origin, the k == i step.
The node-scale GPU tests compare the device with the array forms only."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import global_ref  # noqa: E402
import local_ref  # noqa: E402

F32 = np.float32


def capture(rng, L, res, position, start=(0, 0), keep=0.9, traver_neg=0.05):
    """a capture as local_ref.capture builds it, without the oracle: a random subset of the L^2 cells, records at their positions"""
    lin = np.flatnonzero(rng.random(L * L) < keep)
    cap = local_ref.Capture(None, lin, L, L * res, res, position, start)
    x, y = cap.positions()
    rec = np.zeros(lin.size, local_ref.POINT)
    rec["x"], rec["y"], rec["pad"] = x.astype(F32), y.astype(F32), 1.0
    rec["z"] = rng.uniform(-1, 1, lin.size).astype(F32)
    rec["r"], rec["g"], rec["b"] = (rng.integers(0, 256, lin.size) for _ in range(3))
    rec["covariance"], rec["intensity"] = rng.uniform(0, 1, lin.size).astype(F32), rng.uniform(0, 100, lin.size).astype(F32)
    t = rng.uniform(0, 1, lin.size).astype(F32)
    t[rng.random(lin.size) < traver_neg] = F32(-0.5)
    t[rng.random(lin.size) < 0.02] = F32(-0.0)
    rec["travers"] = t
    cap.rec = rec
    return cap


SHIFTS = [(1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1)]


def run_both(caps, moves):
    """the same spills through both forms; every spill, replaced count, size and export compared"""
    d, lm = {}, local_ref.LocalMap()
    total = 0
    for cap, (cur, shift) in zip(caps, moves):
        o1, r1 = local_ref.spill(cap, cur, shift, d)
        o2, r2 = local_ref.spill_fast(cap, cur, shift, lm)
        assert o1.tobytes() == o2.tobytes() and r1 == r2 and len(d) == len(lm)
        assert local_ref.export(d).tobytes() == local_ref.export_fast(lm).tobytes()
        total += r1
    return d, total


@pytest.mark.parametrize("seed", range(4))
def test_local_spill_forms_agree_on_a_back_and_forth(seed):
    rng = np.random.default_rng(seed)
    L, res = int(rng.integers(6, 30)), float(rng.choice([0.05, 0.1, 0.25]))
    caps, moves, c = [], [], np.zeros(2)
    for k in range(24):
        sx, sy = SHIFTS[int(rng.integers(8))]
        step = np.array([sx, sy], float) * res * float(rng.integers(1, L))
        if k % 2:
            step = -prev_step                                              # back where it came from: keys written again
        prev_step = step
        cap = capture(rng, L, res, (float(c[0]), float(c[1])), (int(rng.integers(L)), int(rng.integers(L))))
        c = c + step
        caps.append(cap); moves.append(((float(F32(c[0])), float(F32(c[1]))), step.astype(F32)))
    d, replaced = run_both(caps, moves)
    assert replaced > 0 and len(d) > 0


@pytest.mark.parametrize("far,res", [(3.0e6, 0.05), (1.0e8, 0.05), (-4.0e6, 0.1)])
def test_local_spill_forms_agree_on_shared_float_keys(far, res):
    """far from the origin neighbouring cells round to one float key: within one spill the later record wins"""
    rng = np.random.default_rng(int(abs(far)) % 1000)
    L = 24
    caps = [capture(rng, L, res, (far, far / 3), (5, 7), keep=1.0, traver_neg=0.0) for _ in range(3)]
    shift = F32(L * res)
    moves = [((far + shift, far / 3 + shift), (shift, shift)), ((far, far / 3 + 2 * shift), (-shift, shift)), ((far, far / 3), (F32(0), -shift))]
    d, replaced = run_both(caps, moves)
    assert replaced > 0 and len(d) < sum(c.rec.size for c in caps)


def test_local_spill_forms_agree_on_every_record_in_one_key():
    cap = capture(np.random.default_rng(9), 16, 0.05, (0.0, 0.0), keep=1.0, traver_neg=0.0)
    cap.rec["x"], cap.rec["y"] = F32(2.5), F32(-0.0)
    d, replaced = run_both([cap, cap], [((1.0, 1.0), (F32(1.0), F32(1.0))), ((1.0, 1.0), (F32(1.0), F32(1.0)))])
    assert len(d) == 1 and replaced == 2 * cap.rec.size - 1


def stack_of(rng, S, n, kinds):
    out = []
    for s in range(S):
        r = np.zeros(n, global_ref.POINT)
        kind = kinds[s % len(kinds)]
        if kind == "dup":                                                  # a few hundred cells, most hit many times
            r["x"] = (rng.integers(-20, 20, n) * 0.05 + rng.uniform(-0.02, 0.02, n)).astype(F32)
            r["y"] = (rng.integers(-8, 8, n) * 0.05 + rng.uniform(-0.02, 0.02, n)).astype(F32)
        elif kind == "one":                                                # every record in one key
            r["x"], r["y"] = F32(0.011), F32(-0.012)
        elif kind == "own":                                                # every record its own key
            r["x"] = (np.arange(n) % 64 * 0.05 + 0.025).astype(F32)
            r["y"] = (np.arange(n) // 64 * 0.05 + 0.025).astype(F32)
        else:                                                              # NaN and inf keys among duplicates
            r["x"] = (rng.integers(-10, 10, n) * 0.05).astype(F32)
            r["y"] = (rng.integers(-10, 10, n) * 0.05).astype(F32)
            bad = rng.random(n)
            r["x"][bad < 0.1] = np.nan
            r["y"][(bad >= 0.1) & (bad < 0.15)] = np.inf
            r["x"][(bad >= 0.15) & (bad < 0.2)] = -np.inf
            r["y"][(bad >= 0.2) & (bad < 0.22)] = np.nan
        r["z"] = rng.uniform(-1, 2, n).astype(F32)
        r["pad"] = rng.uniform(0, 2, n).astype(F32)
        for f in ("r", "g", "b", "a"):
            r[f] = rng.integers(0, 256, n)
        r["covariance"] = rng.uniform(-0.2, 1.2, n).astype(F32)
        r["covariance"][rng.random(n) < 0.05] = 0.0
        r["covariance"][rng.random(n) < 0.05] = 1.0
        r["intensity"], r["travers"] = rng.uniform(0, 100, n).astype(F32), rng.uniform(0, 1, n).astype(F32)
        out.append(r)
    return out


def same_stacks(a, b):
    return len(a) == len(b) and all(global_ref.same(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("kinds", [("dup",), ("one",), ("own",), ("bad",), ("dup", "one", "own", "bad")])
def test_hash_forms_agree(kinds):
    rng = np.random.default_rng(len(kinds[0]) * 7 + len(kinds))
    for rec in stack_of(rng, 4, 1500, kinds):
        for res in (0.05, 0.1):
            assert global_ref.same(global_ref.export(global_ref.hash_cloud(rec, res)), global_ref.hash_fast(rec, res)[0])


@pytest.mark.parametrize("i,k", [(0, 1), (1, 0), (2, 2), (3, 0), (0, 2)])
def test_pair_step_forms_agree(i, k):
    """including the k == i step (a coincident centre's list) and both sides NaN / inf heavy"""
    base = stack_of(np.random.default_rng(100 + 10 * i + k), 4, 2000, ("dup", "bad", "dup", "own"))
    a, b = [s.copy() for s in base], [s.copy() for s in base]
    fa, fb = global_ref.pair_step(a, i, k, 0.05), global_ref.pair_step_fast(b, i, k, 0.05)
    assert fa == fb and same_stacks(a, b)
    assert fa > 0 or (i, k) == (3, 0)


@pytest.mark.parametrize("seed", range(3))
def test_loop_closure_forms_agree(seed):
    rng = np.random.default_rng(seed)
    S = 6
    base = stack_of(rng, S, 1200, ("dup", "bad", "one", "own", "dup"))
    t = np.zeros((S + 2, 4, 4), F32)
    for s in range(S + 2):
        a = rng.uniform(-0.02, 0.02)
        t[s] = [[np.cos(a), -np.sin(a), 0, rng.uniform(-0.1, 0.1)], [np.sin(a), np.cos(a), 0, rng.uniform(-0.1, 0.1)], [0, 0, 1, 0], [0, 0, 0, 1]]
    # ties, a coincident centre (the k == i step), a centre at the radius, an isolated pair; n_opt above the stack size
    centres = np.array([[0, 0], [3, 4], [4, 3], [0, 0], [0, 5], [40, 0], [41, 0], [90, 0]], F32)
    a, b = [s.copy() for s in base], [s.copy() for s in base]
    fa = global_ref.loop_closure(a, S + 2, t, centres, 5.0, 0.05)
    fb = global_ref.loop_closure(b, S + 2, t, centres, 5.0, 0.05, fast=True)
    assert fa == fb and fa > 0 and same_stacks(a, b)
