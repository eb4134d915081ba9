"""bn_compute_composite with a batch of tower-typed expressions under deferred folds and hosted write-backs (tests/deferred_states.py):
the states S2 (the fold parked as a claim-group fold) and S4 (the host has folded its copies; the device is one write-back behind).  A
two-job batch whose arena is the case's whole region: one job's OUTPUT is written INTO a live array of the prover, the other's into the
work area -- the shape of tests/test_gpu_compose_tower_deferred.py.  The batch runs behind bn_compute_composite's blanket flush: what
was waiting must have run before the kernel writes (flushed_folds = 1 or hosted_writebacks = 1), the prover must go on with the
oracle's round values, and every byte of the case's region must equal the model."""
import numpy as np
import pytest

import compose_tower_ref as T
import deferred_states as ds

pytestmark = pytest.mark.gpu

STEPS = [("var", 0), ("var", 1), ("const", 0x53), ("mul", 1, 2), ("add", 0, 3)]  # x + 0x53 y at B8, x a B8 column, y a B1 column
LEVELS, OUT_LEVEL = [3, 0], 3
SELECT = [("var", 0), ("var", 1), ("var", 2), ("add", 0, 1), ("mul", 2, 3), ("add", 0, 4)]  # a + s (a + b) at B1


@pytest.fixture(scope="module")
def contexts():
    c = ds.Contexts()
    yield c
    c.close()


@pytest.mark.parametrize("state", ["S2", "S4"])
def test_batch_output_written_into_a_live_array(contexts, oracle, state):
    hal = contexts.get(state)
    box = {}

    def stage(pv, st):
        live = pv.live[0]
        out = ds.Buf(st, live.off, live.n, "live0")
        n = out.n * 16  # B8 values of the live array
        rng = np.random.default_rng([0xDEFB, len(state)])
        cols = [(T.random_values(rng, 3, n), 3), (T.random_values(rng, 0, n), 0)]
        m = 1 << 9  # the second job: 2^9 bits, four elements of the work area
        bits = [(T.random_values(rng, 0, m), 0) for _ in range(3)]
        ins = []
        for (v, lv), name in zip(cols + bits, ("x", "y", "a", "b", "s")):
            packed = T.pack(v, lv)
            b = st.take(packed.shape[0], "tower input " + name)
            b.host[:] = packed
            ins.append(b)
        side = st.take(4, "second output")
        box.update(out=out, side=side, ins=ins, n=n, m=m, want=T.evaluate_packed(STEPS, cols, OUT_LEVEL), want_side=T.evaluate_packed(SELECT, bits, 0))

    st = ds.reach(hal, oracle, state, seed=0xC7B + len(state), stage=stage)
    members = [hal.expr_compile_tower(SELECT, [0, 0, 0], 0), hal.expr_compile_tower(STEPS, LEVELS, OUT_LEVEL)]
    # rows: a b s x y; the arena is the region, an out_offset an element of it
    jobs = [(0, 0, box["m"].bit_length() - 1, box["side"].off), (1, 3, box["n"].bit_length() - 1, box["out"].off)]
    batch = hal.expr_compile_tower_batch(members, jobs)
    try:
        before, cc, old = hal.group_counters(), hal.compute_composite_batch_counters(), hal.compute_composite_counters()
        rows = [b.dev for b in box["ins"][2:] + box["ins"][:2]]
        hal.compute_composite_tower_batch(rows, st.region, batch)
        d = ds.moved(before, hal.group_counters())
        assert ds.moved(cc, hal.compute_composite_batch_counters()) == {"calls": 1, "launches": 1, "jobs": 2, "programs": 2}
        assert hal.compute_composite_counters() == old
        box["out"].host[:] = box["want"]
        box["side"].host[:] = box["want_side"]
        assert np.array_equal(hal.copy_d2h(box["out"].dev), box["out"].host), "the live array does not hold the expression's values"
        assert np.array_equal(hal.copy_d2h(box["side"].dev), box["side"].host), "the second job's output differs"
        # it writes a live array: what was waiting has run
        if state == "S2":
            assert d.get("flushed_folds", 0) == 1, d
        else:
            assert d.get("hosted_writebacks", 0) == 1, d
        st.continuation()
        st.check_bytes()
    finally:
        for e in members + [batch]:
            hal._exprs.remove(e)
            e.free()
