"""bpgpu_r1cs_constraints_satisfied / _dev and bpgpu_mpc_constraints_eval -- witnesses checked against their constraint rows on the
device -- against Python integers (tests/satisfied_cases.py): every row length around the lazy sums' reductions and the route
threshold in one launch, the edges of the grid, which row / gate / proof is reported, parametric circuits, the device form, two
contexts on one handle, the check beside the prover it guards, and the two-party evaluation opened with its MAC check.
Run with `-m gpu` on an MI355X."""
import ctypes as C
import threading

import pytest

import circuit_gen as cg
import mpc_dealer as md
import oracle_lib as o
import satisfied_cases as sc

pm = cg.pm
N = sc.N
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import mpc_bulletproof_amd as m
    g = m.BpGpu(0)
    yield g
    g.close()


def handle(gpu, rows, n, m, nchi=0):
    rp, kd, ix, cf = sc.csr(rows, nchi)
    if nchi:
        return gpu.circuit_create_param(len(rows), nchi, rp, kd, ix, cf, n, m)
    return gpu.circuit_create(rp, kd, ix, cf, n, m)


def check(gpu, h, rows, wits, chis=None):
    """the host form on a batch equals the model in all four results -> the model's (ok, first_bad_row, first_bad_gate)"""
    ok, row, gate, es = sc.expect(rows, wits, chis)
    got = gpu.r1cs_constraints_satisfied(h, len(wits), len(rows), *sc.planes(wits), gadget_challenges=sc.chi_bytes(chis), want_residuals=True)
    assert got[3] == sc.res_bytes(es)
    assert got[:3] == (ok, row, gate)
    return ok, row, gate


def run(gpu, rows, n, m, wits, chis=None, nchi=0):
    h = handle(gpu, rows, n, m, nchi)
    try:
        return check(gpu, h, rows, wits, chis)
    finally:
        gpu.circuit_destroy(h)


def bumped(wit, by):
    """the witness with its first value moved by `by` (v[0], or a_L[0] with a_O following it: the gates stay satisfied)"""
    w = wit.copy()
    if by and w.v:
        w.v[0] = (w.v[0] + by) % N
    elif by:
        w.a_L[0] = (w.a_L[0] + by) % N
        w.a_O[0] = w.a_L[0] * w.a_R[0] % N
    return w


# ------------------------------------------------------------------------------------------------ row lengths, both routes
def test_every_row_length_in_one_launch(gpu):
    """rows of 0 .. 257 terms and of T - 1, T, T + 1 for the route threshold T in ONE circuit: residuals, first bad row, gates and ok
    equal the model for three provers (the hand-built witness with values at 0, 1 and n - 1, one with other values, one whose a_O is
    wrong at the last multiplier)"""
    T = sc.lane_max()
    rows, wit = sc.length_rows(T)
    n, mm = len(wit.a_L), len(wit.v)
    other = sc.Witness([(x * 7 + 1) % N for x in wit.a_L], wit.a_R, [(x + 5) % N for x in wit.v])
    wrong = wit.copy()
    wrong.a_O[n - 1] = (wrong.a_O[n - 1] + 1) % N
    ok, row, gate = run(gpu, rows, n, mm, [wit, other, wrong])
    assert ok == [0, 0, 0] and gate == [-1, -1, n - 1] and all(r >= 0 for r in row)


# ------------------------------------------------------------------------------------------------ grid edges
@pytest.mark.parametrize("q,nb,n,m", sc.GRID, ids=lambda x: str(x))
def test_grid_edges(gpu, q, nb, n, m):
    """q at 1 and around a block of rows, nb at 1, 3 and past a wave, n from 0, m = 0 with v NULL: prover 0 holds the circuit's
    witness, prover p > 0 the witness with its first value moved by p"""
    circ = sc.grid_circuit(q, n, m)
    wits = [bumped(sc.witness_of(circ), p) for p in range(nb)]
    assert (sc.planes(wits)[3] is None) == (m == 0)
    ok, row, gate = run(gpu, circ.rows, n, m, wits)
    assert ok[0] == 1 and gate == [-1] * nb


# ------------------------------------------------------------------------------------------------ which row, which proof
@pytest.mark.parametrize("bad", ((0,), (254,), (17, 200), ()), ids=("first", "last", "two", "none"))
def test_the_smallest_failing_row_is_reported(gpu, bad):
    circ = sc.grid_circuit(255, 1, 0)
    ok, row, gate = run(gpu, sc.with_constant(circ.rows, *bad), 1, 0, [sc.witness_of(circ)] * 3)
    assert row == [min(bad) if bad else -1] * 3 and ok == [int(not bad)] * 3


@pytest.mark.parametrize("who", ("first", "last", "none"))
def test_the_failing_proof_is_reported(gpu, who):
    q, nb, n, m = 256, 65, 64, 2
    circ = sc.grid_circuit(q, n, m)
    broken = {"first": 0, "last": nb - 1, "none": None}[who]
    wits = [bumped(sc.witness_of(circ), 1 if p == broken else 0) for p in range(nb)]
    ok, row, gate = run(gpu, circ.rows, n, m, wits)
    assert ok == [int(p != broken) for p in range(nb)]
    assert all((r >= 0) == (p == broken) for p, r in enumerate(row))


# ------------------------------------------------------------------------------------------------ gates
@pytest.mark.parametrize("rows_broken", (False, True), ids=("rows-satisfied", "rows-broken"))
@pytest.mark.parametrize("n", (64, 65))
def test_a_wrong_product_is_reported_by_its_multiplier(gpu, n, rows_broken):
    """a_O wrong at i = 0 (prover 0), at i = n - 1 (prover 1), at both (prover 2), nowhere (prover 3); with a broken row beside it the
    two indices are reported independently"""
    circ = sc.grid_circuit(1, n, 2)
    used = {var for row in circ.rows for var, _ in row}
    assert ("O", 0) not in used and ("O", n - 1) not in used           # the wrong products reach no row
    rows = sc.with_constant(circ.rows, 0) if rows_broken else circ.rows
    wits = []
    for where in ((0,), (n - 1,), (0, n - 1), ()):
        w = sc.witness_of(circ)
        for i in where:
            w.a_O[i] = (w.a_O[i] + 1) % N
        wits.append(w)
    ok, row, gate = run(gpu, rows, n, 2, wits)
    assert gate == [0, n - 1, 0, -1] and row == [0 if rows_broken else -1] * 4
    assert ok == [0, 0, 0, int(not rows_broken)]


# ------------------------------------------------------------------------------------------------ parametric circuits
@pytest.mark.parametrize("spec", sc.PARAM, ids=lambda s: "nchi%d" % s[5])
def test_parametric_circuits(gpu, spec):
    """two-phase generated circuits: satisfied for random chi, chi = 0 and chi = n - 1 (one prover each); broken() is reported at its
    first constant row for each of them"""
    circ = cg.Circuit(*spec)
    chis = [[(7919 * (j + 3) + spec[0]) % N for j in range(circ.nchi)], [0] * circ.nchi, [N - 1] * circ.nchi]
    wits = [sc.witness_of(circ)] * 3
    assert run(gpu, circ.rows, circ.n, circ.m, wits, chis, circ.nchi)[0] == [1, 1, 1]
    first_const = next(r for r, row in enumerate(circ.rows) if any(var == sc.ONE for var, _ in row))
    ok, row, gate = run(gpu, circ.broken().rows, circ.n, circ.m, wits, chis, circ.nchi)
    assert ok == [0, 0, 0] and row == [first_const] * 3


def test_a_fault_in_a_chi_block_shows_at_chi_one_only(gpu):
    circ = cg.Circuit(*sc.PARAM[1])
    rows, r = sc.chi_fault(circ)
    chis = [[0] * circ.nchi, [1] * circ.nchi]
    ok, row, gate = run(gpu, rows, circ.n, circ.m, [sc.witness_of(circ)] * 2, chis, circ.nchi)
    assert ok == [1, 0] and row == [-1, r]


# ------------------------------------------------------------------------------------------------ forms
def _dev_call(gpu, h, nb, q, ops, chi, optional):
    """the device form on fresh buffers -> (ok, first_bad_row, first_bad_gate, residuals | None, input flag)"""
    d = [gpu.to_device(b) if b is not None else None for b in ops + (chi,)]
    outs = [gpu.malloc(4 * nb)] + ([gpu.malloc(8 * nb), gpu.malloc(8 * nb), gpu.malloc(32 * nb * q)] if optional else [None] * 3)
    try:
        gpu.r1cs_constraints_satisfied_dev(h, nb, d[0], d[1], d[2], outs[0], d_v=d[3], d_gadget_challenges=d[4], d_first_bad_row=outs[1],
                                           d_first_bad_gate=outs[2], d_residuals=outs[3])
        flag = gpu.input_flag()
        ok = list((C.c_int32 * nb).from_buffer_copy(gpu.download(outs[0], 4 * nb)))
        if not optional:
            return ok, None, None, None, flag
        row = list((C.c_int64 * nb).from_buffer_copy(gpu.download(outs[1], 8 * nb)))
        gate = list((C.c_int64 * nb).from_buffer_copy(gpu.download(outs[2], 8 * nb)))
        return ok, row, gate, gpu.download(outs[3], 32 * nb * q), flag
    finally:
        for p in d + outs:
            if p is not None:
                gpu.free(p)


def test_dev_form_equals_the_host_form_and_a_bad_limb_is_flagged(gpu):
    import mpc_bulletproof_amd as mm
    circ = cg.Circuit(*sc.PARAM[1])
    rows = sc.with_constant(circ.rows, 3)
    wits = [sc.witness_of(circ), bumped(sc.witness_of(circ), 1), sc.witness_of(circ)]
    wits[2].a_O[1] = (wits[2].a_O[1] + 1) % N
    chis = [[5 + p + j for j in range(circ.nchi)] for p in range(3)]
    ops, chi, q = sc.planes(wits), sc.chi_bytes(chis), len(rows)
    h = handle(gpu, rows, circ.n, circ.m, circ.nchi)
    try:
        host = check(gpu, h, rows, wits, chis)
        assert gpu.r1cs_constraints_satisfied(h, 3, q, *ops, gadget_challenges=chi)[:3] == host      # residuals NULL
        ok, row, gate, res, flag = _dev_call(gpu, h, 3, q, ops, chi, True)
        assert flag == 0 and (ok, row, gate) == host and res == sc.res_bytes(sc.expect(rows, wits, chis)[3])
        assert _dev_call(gpu, h, 3, q, ops, chi, False) == (host[0], None, None, None, 0)          # every optional result NULL
        # a_R[1] of prover 0 := the group order: not a canonical limb set; likewise a gadget challenge
        bad_R = ops[1][:32] + N.to_bytes(32, "little") + ops[1][64:]
        bad_ops = (ops[0], bad_R, ops[2], ops[3])
        assert _dev_call(gpu, h, 3, q, bad_ops, chi, True)[4] == 1
        assert _dev_call(gpu, h, 3, q, ops, N.to_bytes(32, "little") + chi[32:], False)[4] == 1
        for kw in (dict(ops=bad_ops, chi=chi), dict(ops=ops, chi=N.to_bytes(32, "little") + chi[32:])):
            with pytest.raises(mm.lib.BpGpuError) as e:
                gpu.r1cs_constraints_satisfied(h, 3, q, *kw["ops"], gadget_challenges=kw["chi"])
            assert e.value.code == mm.lib.E_ARG
        # the handle's view is cached: the same call again, the same answer
        assert gpu.r1cs_constraints_satisfied(h, 3, q, *ops, gadget_challenges=chi, want_residuals=True)[:3] == host
        assert _dev_call(gpu, h, 3, q, ops, chi, True)[:3] == host
    finally:
        gpu.circuit_destroy(h)


def test_refusals_on_a_live_context(gpu):
    import mpc_bulletproof_amd as mm
    E = mm.lib
    circ = cg.Circuit(*sc.PARAM[0])
    hp = handle(gpu, circ.rows, circ.n, circ.m, circ.nchi)
    num = sc.grid_circuit(1, 1, 0)
    hn = handle(gpu, num.rows, 1, 0)
    ok = (C.c_int32 * 4)()
    try:
        f = E._lib.bpgpu_r1cs_constraints_satisfied
        buf = bytes(32 * 64)
        assert f(gpu.ctx, hp, 1, buf, buf, buf, buf, None, ok, None, None, None) == E.E_ARG       # parametric, no challenges
        assert f(gpu.ctx, hn, 1, buf, buf, buf, None, buf, ok, None, None, None) == E.E_ARG       # numeric, challenges
        assert f(gpu.ctx, hn, 1, buf, None, buf, None, None, ok, None, None, None) == E.E_ARG     # a missing plane
        assert f(gpu.ctx, hn, 1, buf, buf, buf, None, None, None, None, None, None) == E.E_ARG    # no ok
        assert f(gpu.ctx, hn, 0, None, None, None, None, None, None, None, None, None) == 0        # nb == 0
        assert E._lib.bpgpu_mpc_constraints_eval(gpu.ctx, hp, 1, buf, buf, buf, buf, None, buf) == E.E_ARG
        assert check(gpu, hn, num.rows, [sc.witness_of(num)]) == ([1], [-1], [-1])                  # and the context still works
    finally:
        gpu.circuit_destroy(hp)
        gpu.circuit_destroy(hn)


def test_two_contexts_share_one_handle_from_two_threads(gpu):
    """the first calls on a fresh handle come from two contexts at once: the one-time build of its view is the handle's own business"""
    import mpc_bulletproof_amd as m
    T = sc.lane_max()
    rows, wit = sc.length_rows(T)
    n, mm = len(wit.a_L), len(wit.v)
    wits = [wit, bumped(wit, 3)]
    want = sc.expect(rows, wits)
    other = m.BpGpu(0)
    h = handle(gpu, rows, n, mm)
    results, errors = {}, []

    def work(name, g):
        try:
            results[name] = [g.r1cs_constraints_satisfied(h, 2, len(rows), *sc.planes(wits), want_residuals=True) for _ in range(3)]
        except Exception as e:      # noqa: BLE001
            errors.append((name, e))
    try:
        threads = [threading.Thread(target=work, args=(name, g)) for name, g in (("a", gpu), ("b", other))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for name in ("a", "b"):
            for got in results[name]:
                assert got == (want[0], want[1], want[2], sc.res_bytes(want[3])), name
    finally:
        gpu.circuit_destroy(h)
        other.close()


# ------------------------------------------------------------------------------------------------ what the check is for
def test_the_check_agrees_with_proving_and_verifying(gpu):
    """five provers of the 8-bit range circuit, prover 3 with a flipped bit in its witness: ok = [1, 1, 1, 0, 1] from the check, and
    bpgpu_r1cs_prove_fs_dev on the SAME device buffers followed by verification gives the same five accept bits"""
    import random
    nb, nbits, cap = 5, 8, 8
    rnd = random.Random(88)
    provers, V, states, init = [], [], b"", b""
    for p in range(nb):
        tr = pm.Transcript(b"RangeProofTest")
        init += tr.state                                       # the verifier starts where Prover::new does
        pv = pm.Prover(pm.PedersenGens(), tr)
        v = rnd.getrandbits(nbits)
        com, var = pv.commit(v, rnd.randrange(N))
        pm.range_proof_gadget(pv, pm.lc_var(var), v, nbits)
        provers.append(pv)
        V.append([com])
        states += pv.transcript.state
    n, m, k = nbits, 1, 3
    rows = [list(lc.items()) for lc in provers[0].constraints]
    wits = [sc.Witness(pv.a_L, pv.a_R, pv.v, pv.a_O) for pv in provers]
    wits[3].a_L[2] = (wits[3].a_L[2] + 1) % N                  # a bit that is no bit: rows and the gate both notice
    want = [1, 1, 1, 0, 1]
    assert sc.expect(rows, wits)[0] == want
    gens = gpu.gens_create(o.gens("G", cap), o.gens("H", cap), o.generator(), o.generator(), 8)
    h = handle(gpu, rows, n, m)
    aL, aR, aO, vv = sc.planes(wits)
    ops = dict(states=states, a_L=aL, a_R=aR, a_O=aO, v=vv, vb=b"".join(md.mont(pv.v_blinding[0]) for pv in provers),
               bl=b"".join(md.mont(rnd.randrange(N)) for _ in range(8 * nb)), keys=bytes(rnd.getrandbits(8) for _ in range(32 * nb)))
    d = {key: gpu.to_device(b) for key, b in ops.items()}
    nvar = 11 + 2 * k
    outs = {"ok": gpu.malloc(4 * nb), "pts": gpu.malloc(64 * nb * nvar), "sc": gpu.malloc(160 * nb)}
    try:
        gpu.r1cs_constraints_satisfied_dev(h, nb, d["a_L"], d["a_R"], d["a_O"], outs["ok"], d_v=d["v"])
        gpu.r1cs_prove_fs_dev(gens, h, nb, d["states"], d["a_L"], d["a_R"], d["a_O"], d["bl"], outs["pts"], outs["sc"], d_v_blinding=d["vb"],
                              d_vector_keys=d["keys"])
        assert gpu.input_flag() == 0
        assert list((C.c_int32 * nb).from_buffer_copy(gpu.download(outs["ok"], 4 * nb))) == want
        pts, scal = gpu.download(outs["pts"], 64 * nb * nvar), gpu.download(outs["sc"], 160 * nb)
        full = b""
        for p in range(nb):
            pp = pts[64 * nvar * p:64 * nvar * (p + 1)]
            full += pp[:6 * 64] + b"".join(pm.p2b(x) for x in V[p]) + pp[6 * 64:]
        assert gpu.r1cs_verify_batch_fs(gens, h, nb, n, k, m, init, full, scal)[0] == want
    finally:
        for p in list(d.values()) + list(outs.values()):
            gpu.free(p)
        gpu.circuit_destroy(h)
        gpu.gens_destroy(gens)


# ------------------------------------------------------------------------------------------------ two parties
def _two_party(gpu, rows, n, m, wits, chis=None, nchi=0):
    """planes dealt by the dealer, each party's bpgpu_mpc_constraints_eval, the rows opened with the MAC and modifier checks ->
    (opened values [p][r], the parties' raw planes [party][p][k][r], the dealer)"""
    dealer = md.Dealer(4242)
    nb, q = len(wits), len(rows)
    dealt = [{key: dealer.share_vec(getattr(w, key)) for key in ("a_L", "a_R", "a_O", "v")} for w in wits]
    h = handle(gpu, rows, n, m, nchi)
    try:
        out = []
        for party in range(2):
            ops = [md.pack([[dealt[p][key][party][k] for k in range(3)] for p in range(nb)]) or None for key in ("a_L", "a_R", "a_O", "v")]
            res = gpu.mpc_constraints_eval(h, nb, q, *ops, gadget_challenges=sc.chi_bytes(chis))
            vals = [md.unmont(b) for b in md.cut(res, 32)]
            out.append([[vals[(3 * p + k) * q:(3 * p + k + 1) * q] for k in range(3)] for p in range(nb)])
    finally:
        gpu.circuit_destroy(h)
    opened = [[dealer.open_sc("row %d of proof %d" % (r, p), [tuple(out[party][p][k][r] for k in range(3)) for party in range(2)])
               for r in range(q)] for p in range(nb)]
    return opened, out, dealer


@pytest.mark.parametrize("broken", (False, True), ids=("satisfied", "broken"))
@pytest.mark.parametrize("kind", ("one-phase", "parametric"))
def test_two_parties_open_the_models_rows(gpu, kind, broken):
    if kind == "parametric":
        circ = cg.Circuit(*sc.PARAM[1])
        chis = [[(31 * (p + 2) + j) % N for j in range(circ.nchi)] for p in range(2)]
    else:
        circ = cg.Circuit(77, 5, 0, 2, 70, 0, "dense+dups")
        chis = None
    rows = circ.broken().rows if broken else circ.rows
    wits = [sc.witness_of(circ), sc.witness_of(circ)]
    opened, _, dealer = _two_party(gpu, rows, circ.n, circ.m, wits, chis, circ.nchi)
    assert dealer.bad == [] and dealer.mod_mismatch == []
    want = sc.expect(rows, wits, chis)[3]
    assert opened == want
    assert any(any(e) for e in want) == broken


def test_two_parties_on_every_row_length(gpu):
    """the hand-built rows of every length (both routes, constants among the terms) on shares: the opened rows are the model's"""
    rows, wit = sc.length_rows(sc.lane_max())
    wits = [wit, bumped(wit, 9)]
    opened, _, dealer = _two_party(gpu, rows, len(wit.a_L), len(wit.v), wits)
    assert dealer.bad == [] and dealer.mod_mismatch == []
    assert opened == sc.expect(rows, wits)[3]


def test_constants_go_to_the_modifier_plane_only(gpu):
    """a circuit of `One` terms only: the share and MAC planes are zero and the modifier plane holds the constant, at both parties"""
    T = sc.lane_max()
    rows = [[(sc.ONE, 5)], [(sc.ONE, 0)], [(sc.ONE, N - 1), (sc.ONE, 3)], [], [(sc.ONE, 2)] * (T + 1)]
    want = [5, 0, 2, 0, 2 * (T + 1)]
    opened, out, dealer = _two_party(gpu, rows, 0, 0, [sc.Witness([], [], [])] * 2)
    assert dealer.bad == [] and dealer.mod_mismatch == [] and opened == [want, want]
    for party in range(2):
        for p in range(2):
            assert out[party][p][0] == [0] * 5 and out[party][p][1] == [0] * 5 and out[party][p][2] == want
