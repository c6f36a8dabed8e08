"""The circuit generator of the GPU circuit tests (tests/circuit_gen.py) against the Python model, without a GPU: its circuits are
provable and verifiable, a broken constant is caught, and the CSR arrays it hands to the library mean what the model's constraint
system means -- repeated variables, explicit zeros, empty rows and the block layout of parametric circuits included."""
import random

import pytest

import circuit_gen as cg
import mpc_dealer as md

pm = cg.pm
N = pm.N


def csr_flatten(q, rp, kd, ix, cf, n, m, z, chi=()):
    """flattened_constraints read off the CSR arrays alone: block j of the rows is weighted by chi_j (block 0 by 1)"""
    w = [[0] * n, [0] * n, [0] * n, [0] * m, [0]]
    for blk, mult in enumerate([1] + list(chi)):
        for r in range(q):
            zr = pow(z, r + 1, N) * mult
            for t in range(rp[blk * q + r], rp[blk * q + r + 1]):
                c = int.from_bytes(cf[32 * t:32 * t + 32], "little")
                w[kd[t]][ix[t]] = (w[kd[t]][ix[t]] + (zr * c if kd[t] < 3 else -zr * c)) % N
    return w[0], w[1], w[2], w[3], w[4][0]


@pytest.mark.parametrize("seed,n1,n2,m,q,nchi,profile", [
    (1, 3, 0, 2, 7, 0, "sparse"),
    (2, 1, 0, 1, 1, 0, "dense"),
    (3, 5, 0, 0, 12, 0, "dups+holes"),
    (4, 2, 2, 1, 8, 2, "sparse+edge_coeff+dups"),
    (5, 3, 0, 2, 40, 0, "columns+edge_coeff"),
    (6, 2, 1, 2, 6, 0, "dense"),
])
def test_model_proves_and_verifies_generated_circuits(seed, n1, n2, m, q, nchi, profile):
    circ = cg.Circuit(seed, n1, n2, m, q, nchi, profile)
    gens = pm.BulletproofGens(8)
    proof, info = cg.prove(circ, gens, seed)
    assert info["chi"] is not None and len(info["chi"]) == nchi
    vf, vinfo = cg.verifier(circ, info["V"])
    assert vf.verify(proof, gens)
    assert vinfo["chi"] == info["chi"]
    # one constant off by one: the witness no longer satisfies the circuit (the prover never reads the constants, so the proof is
    # the same one), and the verifier of that circuit rejects it
    vf, _ = cg.verifier(circ.broken(), info["V"])
    assert not vf.verify(proof, gens)


SHAPES = [(prof, n1, n2, m, q, nchi) for prof in cg.PROFILES for (n1, n2, m, q, nchi) in ((5, 0, 3, 7, 0), (13, 0, 11, 70, 0), (4, 3, 2, 9, 3))]
SHAPES += [("columns+edge_coeff", 13, 0, 11, 300, 0), ("columns+holes", 11, 2, 10, 300, 2), ("dense+dups+edge_coeff", 6, 2, 0, 5, 8),
           ("sparse", 0, 0, 0, 3, 0), ("dense", 1, 0, 0, 1, 0), ("holes", 1, 0, 1, 1, 0), ("sparse", 3, 0, 2, 0, 0)]


@pytest.mark.parametrize("profile,n1,n2,m,q,nchi", SHAPES)
def test_csr_arrays_mean_what_the_model_means(profile, n1, n2, m, q, nchi):
    rnd = random.Random(q + n1)
    circ = cg.Circuit(17 + q, n1, n2, m, q, nchi, profile)
    n = n1 + n2
    for z in (1, 2, N - 1, rnd.randrange(N)):
        chi = [rnd.choice((0, N - 1, rnd.randrange(N))) for _ in range(nchi)]
        want = cg.model_weights(circ, z, chi)
        assert csr_flatten(q, *circ.csr_param(), n, m, z, chi) == want
        if nchi == 0:
            rp, kd, ix, cf = circ.csr()
            assert len(rp) == q + 1 and csr_flatten(q, rp, kd, ix, cf, n, m, z) == want
            ark = circ.csr(ark=True)
            assert ark[:3] == (rp, kd, ix) and [md.unmont(x) for x in md.cut(ark[3], 32)] == [int.from_bytes(x, "little") for x in md.cut(cf, 32)]
        # the rows with the challenges substituted: one more statement of the same circuit
        rp, kd, ix, cf, _ = md.circuit_rows(circ.rows_at(chi))
        assert csr_flatten(q, rp, kd, ix, cf, n, m, z) == want


def _columns(circ):
    rp, kd, ix, cf = circ.csr_param()
    count = {}
    for k, i in zip(kd, ix):
        var = ("LROV"[k], i) if k < 4 else cg.ONE
        count[var] = count.get(var, 0) + 1
    return count


def test_profiles_have_the_shapes_they_promise():
    # columns: one variable of every length in each of L, R, O, V, and the constant column's length is one of them
    for seed in range(10):
        circ = cg.Circuit(seed, 13, 0, 11, 300, 0, "columns+edge_coeff")
        count = _columns(circ)
        for k in "LROV":
            assert {v for var, v in circ.column_lengths.items() if var[0] == k} == set(cg.COLUMN_LENGTHS), k
        for var, length in circ.column_lengths.items():
            assert count.get(var, 0) == length, var
        assert circ.column_lengths[cg.ONE] == cg.COLUMN_LENGTHS[seed % 10]
    # ... also in a parametric circuit: a chosen variable's term lies in one block (a constant has a part in every block it balances)
    circ = cg.Circuit(3, 11, 2, 10, 300, 2, "columns")
    count = _columns(circ)
    assert all(count.get(var, 0) == length for var, length in circ.column_lengths.items() if var != cg.ONE)
    assert 257 in circ.column_lengths.values() and count[cg.ONE] >= circ.column_lengths[cg.ONE]
    # edge_coeff: explicit zeros and the values next to n are there; a worst-case column of 15 or more terms n - 1
    circ = cg.Circuit(1, 13, 0, 11, 300, 0, "columns+edge_coeff")
    rp, kd, ix, cf = circ.csr()
    coeffs = [int.from_bytes(x, "little") for x in md.cut(cf, 32)]
    assert {0, 1, N - 1, N - 2, 1 << 251, (N + 1) // 2} <= set(coeffs)
    per_col = {}
    for k, i, c in zip(kd, ix, coeffs):
        per_col.setdefault((k, i), []).append(c)
    assert any(len(cs) >= 15 and set(cs) == {N - 1} for cs in per_col.values())
    # dups: a variable two to four times in a row, and a group that cancels
    circ = cg.Circuit(2, 6, 0, 3, 40, 0, "dups")
    reps = [max(sum(1 for v, _ in row if v == var) for var, _ in row) for row in circ.rows if row]
    assert max(reps) >= 2 and max(reps) <= 8
    assert any(len(cs) > 1 and sum(cs) % N == 0 for row in circ.rows for cs in [[c for v, c in row if v == row[0][0]]]) or \
        any(sum(c for v, c in row if v == var) % N == 0 and sum(1 for v, _ in row if v == var) > 1 for row in circ.rows for var, _ in row)
    # holes: rows 0 and q - 1 empty, an unused multiplier and commitment, and inside the first wave of 64 rows lanes with and without a constant
    circ = cg.Circuit(4, 9, 0, 5, 300, 0, "holes")
    assert circ.rows[0] == [] and circ.rows[299] == []
    count = _columns(circ)
    assert any(("L", i) not in count and ("R", i) not in count and ("O", i) not in count for i in range(9))
    assert any(("V", i) not in count for i in range(5))
    has_const = [any(v == cg.ONE for v, _ in row) for row in circ.rows[:64]]
    assert 8 < sum(has_const) < 56
