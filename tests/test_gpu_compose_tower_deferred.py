"""bn_compute_composite with a tower-typed expression under deferred folds and hosted write-backs (tests/deferred_states.py): the states
S2 (the fold parked as a claim-group fold) and S4 (the host has folded its copies; the device is one write-back behind), the expression's
OUTPUT written INTO a live array of the prover, exactly as tests/test_gpu_deferred_visibility.py::test_blanket_flush_entry_point does for
the other ops of its table B -- bn_compute_composite is in that table, and the tower route sits behind the same blanket flush.  What was
waiting must have run before the kernel writes (flushed_folds = 1 or hosted_writebacks = 1), the prover must go on with the oracle's
round values, and every byte of the case's region must equal the model."""
import numpy as np
import pytest

import compose_tower_ref as T
import deferred_states as ds

pytestmark = pytest.mark.gpu

STEPS = [("var", 0), ("var", 1), ("const", 0x53), ("mul", 1, 2), ("add", 0, 3)]  # x + 0x53 y at B8, x a B8 column, y a B1 column
LEVELS, OUT_LEVEL = [3, 0], 3


@pytest.fixture(scope="module")
def contexts():
    c = ds.Contexts()
    yield c
    c.close()


@pytest.mark.parametrize("state", ["S2", "S4"])
def test_tower_expression_written_into_a_live_array(contexts, oracle, state):
    hal = contexts.get(state)
    box = {}

    def stage(pv, st):
        live = pv.live[0]
        out = ds.Buf(st, live.off, live.n, "live0")
        n = out.n * 16  # B8 values of the output
        rng = np.random.default_rng([0xDEF, len(state)])
        cols = [(T.random_values(rng, 3, n), 3), (T.random_values(rng, 0, n), 0)]
        ins = []
        for (v, lv), name in zip(cols, ("x", "y")):
            packed = T.pack(v, lv)
            b = st.take(packed.shape[0], "tower input " + name)
            b.host[:] = packed
            ins.append(b)
        box.update(out=out, ins=ins, n=n, want=T.evaluate_packed(STEPS, cols, OUT_LEVEL))

    st = ds.reach(hal, oracle, state, seed=0xC70 + len(state), stage=stage)
    expr = hal.expr_compile_tower(STEPS, LEVELS, OUT_LEVEL)
    try:
        before, cc = hal.group_counters(), hal.compute_composite_counters()
        hal.compute_composite_tower([b.dev for b in box["ins"]], box["out"].dev, expr, box["n"])
        d = ds.moved(before, hal.group_counters())
        assert ds.moved(cc, hal.compute_composite_counters()) == {"calls": 1, "launches": 1, "values": 1}
        box["out"].host[:] = box["want"]
        assert np.array_equal(hal.copy_d2h(box["out"].dev), box["out"].host), "the live array does not hold the expression's values"
        # it writes a live array: what was waiting has run
        if state == "S2":
            assert d.get("flushed_folds", 0) == 1, d
        else:
            assert d.get("hosted_writebacks", 0) == 1, d
        st.continuation()
        st.check_bytes()
    finally:
        hal._exprs.remove(expr)
        expr.free()
