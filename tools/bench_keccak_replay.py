#!/usr/bin/env python
"""Replays the HAL traffic of `constraint_system::prove` for the keccak example prover (BASELINE config 4: examples/keccak.rs,
2^16 permutations) over this backend's C++ mirrors -- the only exercise of configs 1 / 4 there can be without a Rust toolchain
(VERDICT r5 missing 2).  The table and its widths are the reference's (m3/src/gadgets/hash/keccak/stacked.rs:105-151, 292-363):

  * 100 committed columns of 512 bits per permutation (25 state_in + 3 batches x 25 state_out), i.e. 2^(log_perms + 2) elements of
    GF(2^128) each once packed;
  * the constraint set: 75 chi (+ iota) constraints  out - (rc? + b0 + (b1 - 1) b2)  and 25 link constraints
    (out_packed - next_in) * sel, all of degree 2, over 204 multilinears (state_out, b, round constants, packed / shifted columns,
    the selector);
  * piop::prove: ONE BivariateSumcheckProver over the 100 committed multilinears and the ring-switch transparents of their size
    (piop/prove.rs:262-287), every committed column in a claim with the transparent of each evaluation point it is opened at
    (tests/test_gpu_group_wide.py `keccak`: 175 claims over 103 multilinears), FRI interleaved.

Phases, in the order of core/src/constraint_system/prove.rs:74-588 (keccak has no exponentiation and no flushes: prodcheck is empty):

  commit        piop::commit -> commit_interleaved: additive NTT of the merged message + Groestl Merkle tree     (:217-233)
  zerocheck     EqIndSumcheckProver over the old HAL: per round one sumcheck_compute_round_evals with 100 evaluators over 204
                multilinears, the fold of all of them, the fold of the indicator                                  (:431-505)
  ring_switch   per transparent: fill + tensor_expand + fold_right over the 128 one-bit limbs, for THREE transparents (:541-566).
                The reference builds one transparent per claim (ring_switch/prove.rs:127-138: 175 for this claim graph) and, in
                front of them, the partial evaluations of every committed column at its claim's suffix, the tensor algebra per
                prefix and the row-batched evaluations (ring_switch/prove.rs:147-264): this phase leaves all of that out.  The
                faithful phase is bnh_ring_switch_prove (binius_amd/host/ring_switch.hpp); its figure at this shape, beside the
                per-claim sequence, is tools/bench_ring_switch.py -> profiles/r14/ring_switch.json
  piop_prove    prove_interleaved_fri_sumcheck: execute / fold of the 175-claim prover, fri_fold + Merkle on commit rounds (:569-588)

What the replay is NOT: the witness is random (on-device tensor expansions), so the constraints do not hold and the claimed sums
are whatever the columns give -- the provers and kernels do the same arithmetic on the same shapes; the univariate-skip rounds
and the small-field switchover of the reference's zerocheck (which run on its CPU `Backend`, not on the ComputeLayer) are replaced
by the large-field rounds over the packed columns; the evalcheck phase between zerocheck and ring-switch is not replayed.  Its two
device pieces exist behind the C ABI -- bnh_evalcheck_evaluate (the evaluations in front of every round: all leaf columns at their
points in one bn_mle_evaluate_batch, tools/bench_mle_evaluate.py) and bnh_evalcheck_bivariate_prove (one round of the shifted / packed
sumchecks, tools/bench_evalcheck.py) --; the greedy loop with EvalcheckProver's oracle bookkeeping, prove_mlecheck_with_switchover for
composite claims and a phase here that strings them together do not.

Checks: at any size the VERIFIER's equations on what the device produced (zerocheck: every round polynomial sums to the running
claim, the last claim is the batched compositions of the final evaluations times the indicator; piop: RoundProof::recover chain and
the batched products of the final evaluations).  Bit-exact parity of both transcripts with the oracle's restatements at reduced
sizes is tests/test_gpu_zerocheck.py::test_keccak_replay_at_reduced_size, which runs this file's `replay()` with a checker.

`--table u32_add` replays BASELINE config 1 the same way (examples/u32_add.rs: 2^10 additions; m3/src/gadgets/add.rs:25-137 with
commit_zout): 4 committed columns of 32 bits per row (xin, yin, cout, zout), i.e. 2^(log_rows - 2) packed elements each; the
zerocheck over 5 multilinears (the four and cin = cout shifted left by one, a virtual column) with the constraints
carry_out: (xin + cin)(yin + cin) + cin - cout (degree 2) and zout: xin + yin + cin - zout (degree 1 -- evaluated at X = 1 only,
eq_ind.rs:664-668); piop::prove over the 4 committed multilinears and 2 transparents (cout is opened at the zerocheck's point and at
the shifted one): 5 claims.  At this size everything is launch latency -- the line is there so that config 1 has been run, not
for its rate.

  python tools/bench_keccak_replay.py --log-perms 16 [--steps 2]      one JSON line: per-phase ms, kernel ms, launches
  python tools/bench_keccak_replay.py --table u32_add --log-rows 10"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

N_COMMITTED, N_TRANSPARENT = 100, 3  # (the keccak table's)


def keccak_constraints(n_batches=3):
    """(n_multilinears, [(steps, steps of the leading form)]) of the table's constraint set (as tests/test_gpu_hal_wide.py)."""
    evs, n = [], 0
    for _ in range(n_batches):
        out0, b0, rc = n, n + 25, n + 50
        n += 51
        for x in range(5):
            for y in range(5):
                o, bb0, bb1, bb2 = out0 + 5 * y + x, b0 + 5 * y + x, b0 + 5 * y + (x + 1) % 5, b0 + 5 * y + (x + 2) % 5
                steps = [("var", bb1), ("const", 1), ("add", 0, 1), ("var", bb2), ("mul", 2, 3), ("var", bb0), ("add", 4, 5), ("var", o), ("add", 6, 7)]
                if (x, y) == (0, 0):
                    steps += [("var", rc), ("add", 8, 9)]
                evs.append((steps, [("var", bb1), ("var", bb2), ("mul", 0, 1)]))
    sop, nsi, sel = n, n + 25, n + 50
    n += 51
    for i in range(25):
        prod = [("var", sop + i), ("var", nsi + i), ("add", 0, 1), ("var", sel), ("mul", 2, 3)]
        evs.append((prod, prod))
    return n, evs


def piop_claims(c=N_COMMITTED, t=N_TRANSPARENT):
    return [(i, i % t) for i in range(c)] + [(i, (i + 1) % t) for i in range(0, c, 2)] + [(i, (i + 2) % t) for i in range(0, c, 4)]


def u32_add_constraints():
    """zerocheck multilinears 0 xin, 1 yin, 2 cin, 3 cout, 4 zout (m3/src/gadgets/add.rs:95-110; characteristic 2: minus is plus)"""
    prod = [("var", 0), ("var", 2), ("add", 0, 1), ("var", 1), ("var", 2), ("add", 3, 4), ("mul", 2, 5)]
    carry = prod + [("var", 2), ("add", 6, 7), ("var", 3), ("add", 8, 9)]
    zout = [("var", 0), ("var", 1), ("add", 0, 1), ("var", 2), ("add", 2, 3), ("var", 4), ("add", 4, 5)]
    return 5, [(carry, prod), (zout, zout)]


def table(name):
    """the table's shape: one-bit cells per row (log2), committed columns, ring-switch transparents, the zerocheck's multilinears and
    constraints (with their degrees), the PIOP prover's claims (committed index, transparent index)"""
    if name == "keccak":
        n_z, cons = keccak_constraints()
        return dict(name=name, cells_log2=9, n_committed=N_COMMITTED, n_transparent=N_TRANSPARENT, n_z=n_z, constraints=cons, degrees=[2] * len(cons), claims=piop_claims())
    if name == "u32_add":
        n_z, cons = u32_add_constraints()
        return dict(name=name, cells_log2=5, n_committed=4, n_transparent=2, n_z=n_z, constraints=cons, degrees=[2, 1], claims=[(0, 0), (1, 0), (2, 0), (3, 0), (2, 1)])
    raise ValueError("unknown table %r" % name)


def circuit_eval(F, steps, query):
    ev = []
    for s in steps:
        if s[0] == "var":
            ev.append(query[s[1]])
        elif s[0] == "const":
            ev.append(s[1])
        elif s[0] == "add":
            ev.append(ev[s[1]] ^ ev[s[2]])
        elif s[0] == "mul":
            ev.append(F.mul(ev[s[1]], ev[s[2]]))
        else:
            raise ValueError(s)
    return ev[-1]


def horner(F, cs, x):
    e = 0
    for c in reversed(cs):
        e = F.mul(e, x) ^ c
    return e


def device_random(hal, alloc, seed, n_vars):
    from binius_amd import synthetic

    out = alloc.alloc(1 << n_vars)
    hal.fill(out.slice(0, 1), 1 + seed)
    hal.tensor_expand(0, synthetic.random_scalars(seed, n_vars), out)
    return out


class phase:
    """wall clock (device idle at both ends) + per-class kernel time / launches from the context's events"""

    def __init__(self, hal, rec, name, profile):
        self.hal, self.rec, self.name, self.profile = hal, rec, name, profile

    def __enter__(self):
        self.hal.sync()
        if self.profile:
            self.hal.prof_begin()
        self.t0 = time.perf_counter()

    def __exit__(self, *a):
        self.hal.sync()
        ms = (time.perf_counter() - self.t0) * 1e3
        r = self.rec.setdefault(self.name, {})
        r["ms"] = round(min(ms, r.get("ms", ms)), 3)
        if self.profile:
            prof = self.hal.prof_end()
            r["kernel_ms"] = round(sum(v[0] for v in prof.values()), 3)
            r["launches_profiled"] = int(sum(v[1] for v in prof.values()))
            r["by_class"] = {k: [round(v[0], 3), v[1]] for k, v in prof.items() if v[1]}


def replay(args, checker=None):
    """checker (tests only): called with the instance and both transcripts while the context is alive; its dict goes into the record."""
    import numpy as np

    import binius_amd
    from binius_amd import synthetic
    from binius_amd._host import EqIndPlan, FRIParams, PiopCommit, PiopCommittedPlan, PiopPlan, piop_commit_elems

    F = binius_amd.HostField
    tb = table(getattr(args, "table", "keccak"))
    log_rows = args.log_perms if getattr(args, "log_rows", None) is None else args.log_rows
    v = log_rows + tb["cells_log2"] - 7  # (keccak: 512 one-bit cells per row = 4 elements of GF(2^128); u32_add: 32 = a quarter of one)
    if v < 1:
        raise ValueError("the table needs at least 2^%d rows" % (8 - tb["cells_log2"]))
    n = 1 << v
    n_z, cons, degrees, claims_ct = tb["n_z"], tb["constraints"], tb["degrees"], tb["claims"]
    N_COMMITTED, N_TRANSPARENT = tb["n_committed"], tb["n_transparent"]
    total_vars = (N_COMMITTED * n - 1).bit_length()
    arities = []
    while sum(arities) + args.arity < total_vars:
        arities.append(args.arity)
    p = FRIParams(total_vars - args.log_batch, args.log_inv_rate, args.log_batch, arities, n_test_queries=3)
    code_elems = 1 << (total_vars + args.log_inv_rate)
    ml_elems = (N_COMMITTED + N_TRANSPARENT) * n
    arena = (1 << total_vars) + 4 * code_elems + 3 * ml_elems + (n_z + 2) * n + (1 << 18)
    if getattr(args, "merge", "host") == "device":
        arena += code_elems  # (codeword and tree in the caller's buffers; the message's share goes unused)
    rec = {"bench": tb["name"] + "_replay", "log_perms" if tb["name"] == "keccak" else "log_rows": log_rows, "n_vars_packed": v, "committed": N_COMMITTED, "zerocheck": {"multilinears": n_z, "constraints": len(cons)},
           "piop": {"multilinears": N_COMMITTED + N_TRANSPARENT, "claims": len(claims_ct), "total_vars": total_vars,
                    "fri": {"log_inv_rate": args.log_inv_rate, "log_batch": args.log_batch, "arities": arities}}}
    phases = {}
    with binius_amd.Context(0, arena) as hal:
        alloc = hal.dev_alloc()
        committed = [device_random(hal, alloc, 0x6E00 + i, v) for i in range(N_COMMITTED)]
        # ---- the zerocheck's witness: 204 columns (fresh copies: the prover folds them in place); claimed sums from the device
        zc_src = [device_random(hal, alloc, 0x7E00 + j, v) for j in range(min(n_z, 8))]  # (eight distinct columns, copied around)
        zc = [alloc.alloc(n) for _ in range(n_z)]
        eq_scratch = alloc.alloc(n // 2 + 64)
        stream = synthetic.random_scalars(0x2EC0 + v, 2 * v + 1)
        eqc, zch, zbc = stream[:v], stream[v : 2 * v], stream[2 * v]

        def reset_zc():
            for j, d in enumerate(zc):
                hal.copy_d2d(zc_src[j if n_z <= len(zc_src) else (j * 5 + j // 7) % len(zc_src)], d)

        reset_zc()
        # the claimed sums: S_c(0), S_c(1) of the prime polynomial from the old HAL itself (evaluation points 0 and 1), then
        # sum_c = (1 - alpha) S_c(0) + alpha S_c(1) with alpha the first round's coordinate of the indicator's point
        eq_tab = alloc.alloc(max(1, n // 2))
        hal.fill(eq_tab.slice(0, 1), 1)
        hal.tensor_expand(0, eqc[: v - 1], eq_tab)
        exprs = [(hal.compile_expr(c), hal.compile_expr(ci)) for c, ci in cons]
        evs01 = [{"composition": c, "composition_at_infinity": ci, "start": 0, "end": 2, "eq_ind": eq_tab} for c, ci in exprs]
        s01 = hal.hal_round_evals(1, v, None, [("folded", d, 0) for d in zc], evs01, [])
        alpha0 = eqc[v - 1]
        zsums = [F.mul(1 ^ alpha0, a) ^ F.mul(alpha0, b) for a, b in s01]
        for c, ci in exprs:
            c.free()
            ci.free()
        zplan = EqIndPlan(hal, v, zc, cons, zsums, eqc, eq_scratch, zbc, zch, degrees)
        # ---- ring switch inputs
        rs_z = [synthetic.random_scalars(0x3500 + j, v) for j in range(N_TRANSPARENT)]
        rs_vec = alloc.alloc(128)
        hal.copy_h2d(synthetic.random_b128(0x3510, 128), rs_vec)
        rs_evals = [alloc.alloc(n) for _ in range(N_TRANSPARENT)]
        transparents = [alloc.alloc(n) for _ in range(N_TRANSPARENT)]

        def ring_switch():
            for j in range(N_TRANSPARENT):
                hal.fill(rs_evals[j], 0)
                hal.fill(rs_evals[j].slice(0, 1), 0x51 + j)
                hal.tensor_expand(0, rs_z[j], rs_evals[j])
                hal.fold_right(rs_evals[j], 0, rs_vec, transparents[j])

        ring_switch()
        # ---- piop: merged message (host, as the reference merges: reversed order, bit-reversed indices), claims with their true sums;
        # --merge device: no message -- the commit merges the committed columns on the device, straight into the codeword
        merge = getattr(args, "merge", "host")
        rec["merge"] = merge
        if merge == "host":
            msg = np.zeros((1 << total_vars, 2), dtype=np.uint64)
            idx = np.arange(n, dtype=np.int64)
            rev = np.zeros_like(idx)
            for b in range(v):
                rev |= ((idx >> b) & 1) << (v - 1 - b)
            at = 0
            for s in reversed(committed):
                x = hal.copy_d2h(s)
                chunk = np.empty_like(x)
                chunk[rev] = x
                msg[at : at + n] = chunk
                at += n
            d_msg = alloc.alloc(1 << total_vars)
            step = 1 << 22
            for off in range(0, 1 << total_vars, step):
                hal.copy_h2d(msg[off : off + step], d_msg.slice(off, min(1 << total_vars, off + step)))
            del msg
        claims = [(v, i, j, hal.inner_product(committed[i], 7, transparents[j])) for i, j in claims_ct]
        pstream = synthetic.random_scalars(0x7A0 + v, 1 + total_vars)
        pbcs, pchs = pstream[:1], pstream[1:]
        scratch = alloc.alloc(4 * code_elems + ml_elems + (1 << 14))
        if merge == "host":
            pplan = PiopPlan(hal, [(v, s) for s in committed], [(v, s) for s in transparents], claims, p, d_msg, scratch, pbcs, pchs)
        else:
            d_code, d_tree = (alloc.alloc(e) for e in piop_commit_elems(p))
            pcommit = PiopCommit(hal, [(v, s) for s in committed], p, d_code, d_tree)
            pplan = PiopCommittedPlan(hal, [(v, s) for s in committed], [(v, s) for s in transparents], claims, p, d_code, d_tree, scratch, pbcs, pchs)

        for it in range(args.steps + 1):
            profile = it == args.steps  # (the last pass under the event profiler: kernel time and launches; its wall time is not kept)
            tgt = {} if profile else phases
            reset_zc()
            with phase(hal, tgt, "zerocheck", profile):
                zplan.run()
            with phase(hal, tgt, "ring_switch", profile):
                ring_switch()
            c0 = hal.group_counters()
            with phase(hal, tgt, "commit+piop_prove", profile):
                if merge == "host":
                    commit_ms, prove_ms = pplan.run()
                else:
                    pcommit.run(phases=False)
                    commit_ms, prove_ms = pcommit.total_ms, pplan.run()  # (both bracketed inside their calls, as PiopPlan's pair)
            c1 = hal.group_counters()
            if profile:
                for k, r in tgt.items():
                    phases[k].update({kk: vv for kk, vv in r.items() if kk != "ms"})
            else:
                for nm, ms in (("commit", commit_ms), ("piop_prove", prove_ms)):
                    phases.setdefault(nm, {})["ms"] = round(min(ms, phases.get(nm, {}).get("ms", ms)), 3)
        rec["phases"] = phases
        rec["group_counters_piop"] = {k: c1[k] - c0[k] for k in c1}
        rec["total_ms"] = round(phases["zerocheck"]["ms"] + phases["ring_switch"]["ms"] + phases["commit+piop_prove"]["ms"], 3)
        # ---- the verifier's equations on what was timed
        zco, zfin = zplan.round_coeffs(), zplan.final_evals()
        ok_z, running = True, horner(F, zsums, zbc)
        for r in range(v):
            c = zco[r]
            ok_z = ok_z and (c[0] ^ (c[0] ^ c[1] ^ c[2] ^ c[3])) == running
            running = horner(F, c, zch[r])
        acc, pw = 0, 1
        for c, _ in cons:
            acc ^= F.mul(pw, circuit_eval(F, c, zfin[:n_z]))
            pw = F.mul(pw, zbc)
        ok_z = ok_z and F.mul(acc, zfin[n_z]) == running
        items = pplan.transcript()
        proofs = [pl for k, pl in items if k == "round_proof"]
        finals = [pl for k, pl in items if k == "multilinear_evals"]
        ok_p, running = len(proofs) == total_vars and len(finals) == 1, F.mul(pbcs[0], horner(F, [c[3] for c in claims], pbcs[0]))
        # (BatchVerifier, front_loaded.rs:56-230: the prover's claims batched by powers of its coefficient, the whole times the batch
        # coefficient; its round polynomials arrive scaled the same way)
        for r, pr in enumerate(proofs[:v]):
            c0_, c1_ = (pr + [0, 0])[:2]
            c2_ = running ^ c1_  # RoundProof::recover (common.rs:176-182): P(0) + P(1) = sum
            running = horner(F, [c0_, c1_, c2_], pchs[r])
        if ok_p:
            fe = finals[0]
            acc, pw = 0, 1
            for i, j in claims_ct:
                acc ^= F.mul(pw, F.mul(fe[i], fe[N_COMMITTED + j]))
                pw = F.mul(pw, pbcs[0])
            ok_p = F.mul(pbcs[0], acc) == running
        rec["verifier_check"] = {"zerocheck": bool(ok_z), "piop_sumcheck": bool(ok_p)}
        if checker is not None:
            reset_zc()
            rec["oracle_check"] = checker(dict(
                n_vars=v, committed=[hal.copy_d2h(s) for s in committed], transparents=[hal.copy_d2h(s) for s in transparents],
                zerocheck_multilinears=[hal.copy_d2h(s) for s in zc], constraints=cons, degrees=degrees, zerocheck_sums=zsums, eq_ind_challenges=eqc, zerocheck_batch_coeff=zbc,
                zerocheck_challenges=zch, zerocheck_transcript=(zco, zfin), claims=claims, fri_params=p, piop_batch_coeffs=pbcs, piop_challenges=pchs,
                commitment=bytes(pplan.commitment) if merge == "host" else pcommit.commitment, piop_transcript=items))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", choices=["keccak", "u32_add"], default="keccak")
    ap.add_argument("--log-perms", type=int, default=16, help="log2 of the number of permutations (the keccak table's rows); config 4: 16")
    ap.add_argument("--log-rows", type=int, default=None, help="log2 of the table's rows (overrides --log-perms); config 1: --table u32_add --log-rows 10")
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--log-inv-rate", type=int, default=1)
    ap.add_argument("--log-batch", type=int, default=4)
    ap.add_argument("--arity", type=int, default=4)
    ap.add_argument("--merge", choices=["host", "device"], default="host",
                    help="host: numpy merge_multilins + upload + bnh_piop_prove (as every earlier record); device: bnh_piop_commit + bnh_piop_prove_committed")
    rec = replay(ap.parse_args())
    print(json.dumps(rec))
    sys.exit(0 if all(rec["verifier_check"].values()) else 1)


if __name__ == "__main__":
    main()
