"""CPU restatement of the GKR exponentiation argument (core/src/protocols/gkr_exp): the circuit's layers (witness.rs:31-110, 139-156,
258-284), gkr_exp::batch_prove (batch_prove.rs:46-315, provers.rs:20-385, compositions.rs, utils.rs) over a step-wise eq-indicator
sumcheck prover composed from the oracle's pinned pieces the way oracle.zerocheck_ref.eqind_sumcheck_prove composes them, batched by
sumcheck::batch_prove (prove/batch_sumcheck.rs:102-199), and gkr_exp::batch_verify (batch_verify.rs, verifiers.rs, with the verifier side
of the batched sumcheck, verify_sumcheck.rs:30-129) as a checker that shares nothing with the prover.  Pinned by
tests/test_gkr_exp_oracle.py; the GPU parity tests compare with it.

A claim is a dict: n_vars, kind ("static" | "dynamic"), base (an int | a (2^n_vars, 2) array), bits (w arrays of 2^n_vars 0/1 values,
e_0 = the least significant bit first), point (n_vars scalars), eval.  Claims are sorted by n_vars descending.  Everything is
High-to-Low.  Transcript samples: coeffs[L][g] = the batch coefficient of the g-th sumcheck prover of layer L, challenges[L][r] = the
challenge of round r of layer L."""
import numpy as np

import oracle as o
from oracle.zerocheck_ref import interpolate

ONE = 1


# ------------------------------------------------------------------------------------------------ the circuit
def bits_to_b128(bits):
    out = o.arr(len(bits))
    out[:, 0] = np.asarray(bits, dtype=np.uint64)
    return out


def pack_bits(bits):
    """A bit column as a B1 multilinear packed into 16-byte elements: bit i = bit i & 127 of element i >> 7, little-endian."""
    b = np.asarray(bits, dtype=np.uint8)
    padded = np.zeros(max(128, b.shape[0]), dtype=np.uint8)
    padded[: b.shape[0]] = b
    return np.packbits(padded, bitorder="little").view(np.uint64).reshape(-1, 2).copy()


def _select(bits, c):
    """e ? c : 1 per row; c an int or an array."""
    n = len(bits)
    cs = o.ints_to_arr([c] * n) if isinstance(c, int) else c
    out = o.arr(n)
    out[:, 0] = 1
    m = np.asarray(bits, dtype=bool)
    out[m] = cs[m]
    return out


def exp_layers(bits, base, kind):
    """[V_0, ..., V_{w-1}] as (2^n_vars, 2) arrays."""
    w = len(bits)
    layers = []
    if kind == "static":
        c = base
        for k in range(w):
            sel = _select(bits[k], c)
            layers.append(sel if k == 0 else o.mul_vec(layers[-1], sel))
            c = o.mul(c, c)
    else:
        for k in range(w):
            sel = _select(bits[w - 1 - k], base)
            if k == 0:
                layers.append(sel)
            else:
                prev = np.ascontiguousarray(layers[-1])
                layers.append(o.mul_vec(o.mul_vec(prev, prev), sel))
    return layers


# ------------------------------------------------------------------------------------------------ the eq-indicator prover, step-wise
class EqIndProver:
    """EqIndSumcheckProver::{execute, fold, finish} (sumcheck/prove/eq_ind.rs:378-644), High-to-Low, over n_vars >= 0 variables;
    compositions: [(steps, steps of the leading form, degree)] over the concatenated multilinears."""

    def __init__(self, multilins, n_vars, compositions, sums, eq_ind_challenges):
        assert len(eq_ind_challenges) == n_vars
        self.n_vars, self.n_rem = n_vars, n_vars
        self.mls = [x.copy() for x in multilins]
        self.comps = compositions
        self.sums = list(sums)
        self.alphas = list(eq_ind_challenges)
        self.D = max([2] + [d for _, _, d in compositions])
        self.prefix = 1
        self.prime = None
        if n_vars >= 1:
            self.eq = o.arr(1 << (n_vars - 1))
            self.eq[0] = o.ints_to_arr([1])[0]
            o.tensor_expand(self.eq, 0, self.alphas[: n_vars - 1])

    def execute(self, batch_coeff):
        D, n_rem = self.D, self.n_rem
        alpha = self.alphas[n_rem - 1]
        evaluators = [{"steps": c, "steps_inf": ci, "start": 1, "end": 1 + d, "eq_ind": self.eq[: 1 << (n_rem - 1)]} for c, ci, d in self.comps]
        rc, evals = o.hal_round_evals(1, n_rem, None, [("folded", np.ascontiguousarray(x[: 1 << n_rem]), 0) for x in self.mls], evaluators, list(range(2, D)))
        assert rc == 0
        denom_inv = o.invert(1 ^ alpha) if (1 ^ alpha) else 0
        self.prime, batched, scale = [], [0] * (D + 1), 1
        for c, (_, _, d) in enumerate(self.comps):
            y1, yinf = evals[c][0], (evals[c][1] if d >= 2 else 0)
            y0 = o.mul(self.sums[c] ^ o.mul(y1, alpha), denom_inv)
            pc = [y0, y1 ^ y0 ^ yinf, yinf] if d <= 2 else interpolate([y0, y1] + list(evals[c][2:d]), yinf)
            pc = pc + [0] * (D + 1 - len(pc))
            self.prime.append(pc)
            for i in range(D + 1):
                batched[i] ^= o.mul(pc[i], scale)
            scale = o.mul(scale, batch_coeff)
        coeffs = [0] * (D + 2)
        for i in range(D + 1):
            coeffs[i] ^= o.mul(batched[i], 1 ^ alpha)
            coeffs[i + 1] ^= batched[i]
        return [o.mul(v, self.prefix) for v in coeffs]

    def fold(self, z):
        n_rem = self.n_rem
        alpha = self.alphas[n_rem - 1]
        self.prefix = o.mul(self.prefix, alpha ^ z ^ 1)
        self.sums = [o.evaluate_univariate(pc, z) for pc in self.prime]
        half = 1 << (n_rem - 1)
        for x in self.mls:
            lo, hi = np.ascontiguousarray(x[:half]), np.ascontiguousarray(x[half : 2 * half])
            o.extrapolate_line(lo, hi, z)
            x[:half] = lo
        if n_rem - 1 > 0:
            q = half >> 1
            self.eq[:q] ^= self.eq[q:half]
        self.n_rem -= 1

    def finish(self):
        assert self.n_rem == 0
        return [o.arr_to_ints(x[:1])[0] for x in self.mls] + [self.prefix]


def batch_sumcheck_prove(provers, coeffs, challenges):
    """sumcheck::batch_prove (prove/batch_sumcheck.rs:102-199) over provers sorted by n_vars descending: a prover's coefficient
    coeffs[i] is taken when the round with its n_vars begins.  Returns (round proofs, multilinear_evals per prover, the challenges
    reversed)."""
    if not provers:
        return [], [], []
    assert all(a.n_vars >= b.n_vars for a, b in zip(provers, provers[1:])), "ClaimsOutOfOrder"
    n_rounds = provers[0].n_vars
    active, proofs, used = 0, [], []
    for r in range(n_rounds):
        while active < len(provers) and provers[active].n_vars == n_rounds - r:
            active += 1
        acc = []
        for i in range(active):
            pc = [o.mul(v, coeffs[i]) for v in provers[i].execute(coeffs[i])]
            acc += [0] * (len(pc) - len(acc))
            for j, v in enumerate(pc):
                acc[j] ^= v
        proofs.append(acc[:-1])
        used.append(challenges[r])
        for i in range(active):
            provers[i].fold(challenges[r])
    return proofs, [p.finish() for p in provers], used[::-1]


# ------------------------------------------------------------------------------------------------ gkr_exp::batch_prove
def _static_comp(a, b, c):
    return ([("var", a), ("var", b), ("const", c), ("mul", 1, 2), ("const", 1), ("add", 4, 1), ("add", 5, 3), ("mul", 0, 6)],
            [("var", a), ("var", b), ("mul", 0, 1), ("const", c ^ 1), ("mul", 2, 3)], 2)


def _dynamic_comp(a, b, c):
    return ([("var", a), ("var", b), ("var", c), ("pow", 0, 2), ("mul", 1, 2), ("const", 1), ("add", 5, 1), ("add", 6, 4), ("mul", 3, 7)],
            [("var", a), ("var", b), ("var", c), ("pow", 0, 2), ("mul", 1, 2), ("mul", 3, 4)], 4)


def _dynamic_last_comp(a, b):
    return ([("var", a), ("var", b), ("mul", 0, 1), ("const", 1), ("add", 3, 1), ("add", 4, 2)], [("var", a), ("var", b), ("mul", 0, 1)], 2)


def first_layer_inverse(v, g):
    d = g ^ 1
    return o.mul(v ^ 1, o.invert(d) if d else 0)


def exp_prove(claims, coeffs, challenges, layers=None):
    """Returns {"round_proofs": [layer][round][coefficients], "multilinear_evals": [layer][sumcheck prover][evaluations, the
    indicator's last], "layer_claims": [layer][(point, eval)]}; a layer without a sumcheck has empty round_proofs and
    multilinear_evals."""
    assert all(a["n_vars"] >= b["n_vars"] for a, b in zip(claims, claims[1:])), "ClaimsOutOfOrder"
    if layers is None:
        layers = [exp_layers(c["bits"], c["base"], c["kind"]) for c in claims]
    st = [{"c": c, "w": len(c["bits"]), "V": layers[t], "point": list(c["point"]), "eval": c["eval"]} for t, c in enumerate(claims)]
    out = {"round_proofs": [], "multilinear_evals": [], "layer_claims": []}
    max_w = max([s["w"] for s in st] + [0])
    for L in range(max_w):
        # consecutive provers with equal points (batch_prove.rs:123-196)
        groups = []
        for s in st:
            if groups and groups[-1][0]["point"] == s["point"]:
                groups[-1].append(s)
            else:
                groups.append([s])
        provers = []
        for grp in groups:
            mls, comps, sums = [], [], []
            for s in grp:
                c, w, last = s["c"], s["w"], s["w"] - 1 - L == 0
                at = len(mls)
                if c["kind"] == "static":
                    if last:
                        continue
                    k = w - 1 - L
                    power = c["base"]
                    for _ in range(k):
                        power = o.mul(power, power)
                    mls += [s["V"][w - 2 - L], bits_to_b128(c["bits"][k])]
                    comps.append(_static_comp(at, at + 1, power))
                elif last:
                    mls += [c["base"], bits_to_b128(c["bits"][L])]
                    comps.append(_dynamic_last_comp(at, at + 1))
                else:
                    mls += [s["V"][w - 2 - L], bits_to_b128(c["bits"][L]), c["base"]]
                    comps.append(_dynamic_comp(at, at + 1, at + 2))
                sums.append(s["eval"])
            if comps:
                provers.append(EqIndProver(mls, len(grp[0]["point"]), comps, sums, grp[0]["point"]))
        proofs, evals, r = batch_sumcheck_prove(provers, coeffs[L], challenges[L])
        out["round_proofs"].append(proofs)
        out["multilinear_evals"].append(evals)
        flat = [v for e in evals for v in e[:-1]]
        claims_out, at = [], 0
        for s in st:
            c, last = s["c"], s["w"] - 1 - L == 0
            n = len(s["point"])
            if c["kind"] == "static":
                if last:
                    claims_out.append((list(s["point"]), first_layer_inverse(s["eval"], c["base"])))
                    continue
                mine, at = flat[at : at + 2], at + 2
                s["point"], s["eval"] = r[:n], mine[0]
                claims_out.append((r[:n], mine[1]))
            else:
                k = 2 if last else 3
                mine, at = flat[at : at + k], at + k
                claims_out.append((r[:n], mine[1]))
                claims_out.append((r[:n], mine[0] if last else mine[2]))
                if not last:
                    s["point"], s["eval"] = r[:n], mine[0]
        assert at == len(flat)
        out["layer_claims"].append(claims_out)
        st = [s for s in st if s["w"] - 1 - L != 0]
    return out


# ------------------------------------------------------------------------------------------------ gkr_exp::batch_verify
def _eq_eval(x, y):
    r = 1
    for a, b in zip(x, y):
        r = o.mul(r, 1 ^ a ^ b)
    return r


def exp_verify(meta, proof, coeffs, challenges):
    """meta: per claim a dict n_vars, width, kind, base (static: the int), point, eval -- no witness data.  Raises AssertionError where
    the verifier would reject; returns the LayerClaims per layer, from the proof alone."""
    vs = [{"kind": m["kind"], "g": m.get("base"), "w": m["width"], "pt": list(m["point"]), "ev": m["eval"]} for m in meta]
    assert all(len(a["pt"]) >= len(b["pt"]) for a, b in zip(vs, vs[1:])), "ClaimsOutOfOrder"
    result = []
    for L in range(max([v["w"] for v in vs] + [0])):
        runs, i = [], 0
        while i < len(vs):
            j = i
            while j < len(vs) and vs[j]["pt"] == vs[i]["pt"]:
                j += 1
            runs.append(vs[i:j])
            i = j

        def n_mls(v):
            fin = v["w"] == L + 1
            return (0 if fin else 2) if v["kind"] == "static" else (2 if fin else 3)

        runs = [run for run in runs if sum(n_mls(v) for v in run)]
        rounds, evals = proof["round_proofs"][L], proof["multilinear_evals"][L]
        assert len(evals) == len(runs), "layer %d: one evaluation list per sumcheck claim" % L
        n_rounds = max([len(run[0]["pt"]) for run in runs] + [0])
        assert len(rounds) == n_rounds
        claim, seen, degree, ch = 0, 0, 0, []

        def take(claim, seen, degree, n):
            while seen < len(runs) and len(runs[seen][0]["pt"]) == n:
                b, scale = coeffs[L][seen], coeffs[L][seen]
                for v in runs[seen]:
                    if n_mls(v):
                        claim ^= o.mul(scale, v["ev"])
                        scale = o.mul(scale, b)
                        degree = max(degree, 5 if n_mls(v) == 3 else 3)
                seen += 1
            return claim, seen, degree

        for r in range(n_rounds):
            claim, seen, degree = take(claim, seen, degree, n_rounds - r)
            cs = list(rounds[r])
            assert len(cs) == degree, "layer %d round %d: %d coefficients for degree %d" % (L, r, len(cs), degree)
            top = claim
            for v in cs[1:]:
                top ^= v
            z = challenges[L][r]
            claim = o.evaluate_univariate(cs + [top], z)
            ch.append(z)
        claim, seen, degree = take(claim, seen, degree, 0)
        rev = ch[::-1]
        want = 0
        for g, run in enumerate(runs):
            n = len(run[0]["pt"])
            ev = list(evals[g])
            assert len(ev) == sum(n_mls(v) for v in run) + 1
            ind = ev.pop()
            assert ind == _eq_eval(run[0]["pt"], rev[:n]), "layer %d: the indicator's evaluation is not eq(point, challenges)" % L
            b, scale, at, acc = coeffs[L][g], coeffs[L][g], 0, 0
            for v in run:
                k = n_mls(v)
                if not k:
                    continue
                x = ev[at : at + k]
                at += k
                if v["kind"] == "static":
                    c = v["g"]
                    for _ in range(v["w"] - 1 - L):
                        c = o.mul(c, c)
                    val = o.mul(x[0], 1 ^ x[1] ^ o.mul(x[1], c))
                elif k == 2:
                    val = 1 ^ x[1] ^ o.mul(x[1], x[0])
                else:
                    val = o.mul(o.mul(x[0], x[0]), 1 ^ x[1] ^ o.mul(x[1], x[2]))
                acc ^= o.mul(scale, val)
                scale = o.mul(scale, b)
            want ^= o.mul(acc, ind)
        assert want == claim, "layer %d: the final sumcheck claim does not match the evaluations" % L
        # the LayerClaims, and the verifiers' next claims (verifiers.rs finish_layer)
        flat = [x for ev in evals for x in ev[:-1]]
        layer_claims, at = [], 0
        for v in vs:
            k, n = n_mls(v), len(v["pt"])
            if k == 0:
                d = v["g"] ^ 1
                layer_claims.append((list(v["pt"]), o.mul(v["ev"] ^ 1, o.invert(d) if d else 0)))
                continue
            x, at = flat[at : at + k], at + k
            layer_claims.append((rev[:n], x[1]))
            if v["kind"] == "dynamic":
                layer_claims.append((rev[:n], x[0] if k == 2 else x[2]))
            if v["w"] != L + 1:
                v["pt"], v["ev"] = rev[:n], x[0]
        result.append(layer_claims)
        vs = [v for v in vs if v["w"] != L + 1]
    return result
