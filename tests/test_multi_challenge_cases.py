"""tests/multi_challenge_cases.py on the model alone: a circuit whose randomized phase draws several challenges, each under its own
label, proves and verifies; the labels' order matters; distinct labels give other challenges than one label; the two-shuffle gate
program's witness satisfies its circuit.  No GPU needed."""
import pytest

import circuit_gen as cg
import mpc_dealer as md
import multi_challenge_cases as mc

pm = mc.pm
N = mc.N


@pytest.mark.parametrize("shape", mc.SHAPES, ids=lambda s: "n%d+%d-m%d-q%d-chi%d" % s[:5])
def test_model_verifier_accepts_the_model_prover_under_distinct_labels(shape):
    """the record's own verification (labels in draw order) accepted, the verifier drew the prover's challenges, and the challenges
    the device verifier returns (y z u x w r u_1..u_k) extend the prover's (y z u x w u_1..u_k)"""
    circ, r = mc.circuit(shape), mc.record(shape, 0)
    assert len(set(circ.labels)) == circ.nchi == shape[4]
    assert r["accepted"] and r["verifier_chi"] == r["chi"] and len(r["chi"]) == 32 * circ.nchi
    k = mc.lg_padded(circ.n)
    vch, pch = md.cut(r["verifier_challenges"], 32), md.cut(r["challenges"], 32)
    assert len(vch) == 6 + k and vch[:5] + vch[6:] == pch


@pytest.mark.parametrize("shape", mc.SHAPES, ids=lambda s: "n%d+%d-m%d-q%d-chi%d" % s[:5])
def test_swapping_two_labels_on_the_verifier_side_rejects(shape):
    circ, r = mc.circuit(shape), mc.record(shape, 0)
    swapped = list(circ.labels)
    swapped[0], swapped[-1] = swapped[-1], swapped[0]
    ok, _, chi = mc.verify_model(circ, 0, r["V"], r["proof"], labels=swapped)
    assert not ok and chi != r["chi"]


@pytest.mark.parametrize("shape", mc.SHAPES, ids=lambda s: "n%d+%d-m%d-q%d-chi%d" % s[:5])
def test_distinct_labels_draw_other_challenges_than_one_label(shape):
    """the same circuit installed by circuit_gen (every draw under cg.CHI_LABEL) and with draw j under label j, on the same transcript"""
    circ = mc.circuit(shape)
    r = mc.record(shape, 0)

    def drawn(install):
        vf = pm.Verifier(pm.PedersenGens(), pm.Transcript(mc.label(0)))
        info = install(vf, commitments=r["V"])
        vf._create_randomized_constraints()
        return info["chi"]
    one, many = drawn(lambda vf, **kw: cg.Circuit.install(circ, vf, **kw)), drawn(circ.install)
    assert len(one) == len(many) == circ.nchi and len(set(many)) == circ.nchi
    assert all(a != b for a, b in zip(one, many))
    # ... and a circuit told to use one label everywhere draws circuit_gen's
    same = mc.Circuit(circ.seed, circ.n1, circ.n2, circ.m, circ.q, circ.nchi, circ.profile, labels=[cg.CHI_LABEL] * circ.nchi)
    assert same.rows == circ.rows and drawn(same.install) == one


def test_batches_cover_the_wave_boundary_and_share_prover_zero():
    shape = mc.SHAPES[1]
    recs, which = mc.batch(shape, 65)
    assert which == (0, 63, 64) and len(recs) == 65 and recs[63] is mc.record(shape, 63)
    assert "proof" not in recs[1] and recs[1]["a_L2"] == recs[0]["a_L2"] and recs[1]["state_in"] != recs[0]["state_in"]
    assert len({r["init"] for r in recs}) == 65


def test_two_shuffle_program_satisfies_its_circuit_for_any_challenges():
    prog, outs = mc.two_shuffles_program()
    assert (prog.n, prog.phase1, prog.m, prog.nchi) == (6, 0, 10, 2) and outs == [0, 1, 3, 5]
    rows = mc.two_shuffles_rows(prog, outs)
    rp, kd, ix, cf, _ = md.circuit_rows(rows, nchi=2)
    assert len(rp) == 3 * len(rows) + 1
    for chi in ((0, 0), (1, N - 1), (12345, 67890)):
        for wrong in (False, True):
            v = mc.two_shuffles_values(3, wrong)
            aL, aR, aO = prog.evaluate(v, (), chi)
            val = {cg.ONE: 1}
            for i in range(prog.n):
                val[("L", i)], val[("R", i)], val[("O", i)] = aL[i], aR[i], aO[i]
            for i, x in enumerate(v):
                val[("V", i)] = x
            resid = [sum(cg.coeff_at(c, chi) * val[var] for var, c in row) % N for row in rows]
            # the first chain reads chi_1 alone, the second chi_2 alone
            assert aL[0] == (v[1] - chi[0]) % N and aL[2] == (v[6] - chi[1]) % N
            if wrong and chi != (0, 0):
                assert resid[:-1] == [0] * (len(rows) - 1) and resid[-1] != 0
            elif not wrong:
                assert resid == [0] * len(rows)
