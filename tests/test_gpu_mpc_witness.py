"""The two-party witness sessions (bpgpu_mpc_witness_*) on the GPU: two contexts act as the two parties, the test plays the network
(it opens d and e of every level with the MAC and modifier checks), and every byte a party's device returns must be the model's
(tests/mpc_witness_cases.py): the arithmetic is exact in F_n and the outputs are canonical ark limbs, so there is no tolerance.
Run with `-m gpu` on an MI355X."""
import random

import pytest

import mpc_dealer as md
import mpc_witness_cases as mc
import oracle_lib as o
import witness_cases as wc

pytestmark = pytest.mark.gpu
N = mc.N
NBS = (1, 3, 22)          # 22 proofs are 66 virtual provers: more than a wave
NAMES = [c.name for c in mc.cases()]
GADGETS = [c.name for c in mc.gadget_cases()]


@pytest.fixture(scope="module")
def gpus():
    import mpc_bulletproof_amd as m
    two = m.lib.device_count() >= 2
    g = [m.BpGpu(0), m.BpGpu(1 if two else 0)]
    yield g
    for x in g:
        x.close()


@pytest.fixture(scope="module")
def programs(gpus):
    """case name -> the program handle of each party, created once"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = [g.witness_create(*mc.case(name).prog.create_args()) for g in gpus]
        return made[name]
    yield get
    for hs in made.values():
        for g, h in zip(gpus, hs):
            g.witness_destroy(h)


def _checker(mo):
    """a dealer with the model's MAC key and empty records: what this test's openings are checked with"""
    d = md.Dealer(0)
    d.alpha = mo.dealer.alpha
    return d


def _open_masked(chk, masked, nb, G, lvl):
    """masked[party]: nb x 2 x 3 x G ark bytes -> opened nb x 2 x G ark bytes"""
    vals = [[md.unmont(b) for b in md.cut(x, 32)] for x in masked]
    return b"".join(md.mont(chk.open_sc("%s %d[%d][%d]" % ("de"[de], lvl, p, s),
                                        [tuple(vals[q][((p * 2 + de) * 3 + k) * G + s] for k in range(3)) for q in range(2)]))
                    for p in range(nb) for de in range(2) for s in range(G))


def _run(gpus, hw, mo, chk, phase=0, rounds=None, planes_in=None, first_level=0):
    """begin -> per level mask on both parties, open, combine on both -> finish; every masked buffer and the opening against the model"""
    prog, nb = mo.case.prog, mo.nb
    rounds = mo.rounds if rounds is None else rounds
    chi = mo.chi if phase != 1 else None
    sess = [gpus[q].mpc_witness_begin(hw[q], nb, phase, mo.v[q], mo.inputs[q], chi, *(planes_in[q] if planes_in else (None,) * 3))
            for q in range(2)]
    try:
        for at, r in enumerate(rounds):
            G = len(r["gates"])
            for q in range(2):
                assert gpus[q].mpc_witness_levels_left(sess[q]) == len(rounds) - at and gpus[q].mpc_witness_level_len(sess[q]) == G
            masked = [gpus[q].mpc_witness_mask(sess[q], nb, r["triples"][q]) for q in range(2)]
            for q in range(2):
                assert masked[q] == r["masked"][q], (mo.case.name, first_level + at, q)
            opened = _open_masked(chk, masked, nb, G, first_level + at)
            assert opened == r["opened"]
            for q in range(2):
                gpus[q].mpc_witness_combine(sess[q], opened)
        for q in range(2):
            assert gpus[q].mpc_witness_levels_left(sess[q]) == 0 and gpus[q].mpc_witness_level_len(sess[q]) == 0
        return [gpus[q].mpc_witness_finish(sess[q], nb, prog.n) for q in range(2)]
    finally:
        for q in range(2):
            if sess[q] is not None:
                gpus[q].mpc_witness_destroy(sess[q])


def _opened_witness(chk, planes, nb, n):
    """planes[party] = (a_L, a_R, a_O) -> the opened planes, nb x n ark bytes each"""
    return [b"".join(md.mont(x) for row in mc.open_planes(chk, "LRO"[w], [planes[q][w] for q in range(2)], nb, n) for x in row) for w in range(3)]


def _circuits(gpus, case):
    q, nchi, rp, kd, ix, cf = wc.circuit_csr(case)
    prog = case.prog
    return q, [g.circuit_create_param(q, nchi, rp, kd, ix, cf, prog.n, prog.m) if nchi else g.circuit_create(rp, kd, ix, cf, prog.n, prog.m)
               for g in gpus]


def _residuals(gpus, circs, q, mo, chk, planes):
    res = [gpus[p].mpc_constraints_eval(circs[p], mo.nb, q, *planes[p], v=mo.v[p], gadget_challenges=mo.chi) for p in range(2)]
    return mc.open_planes(chk, "row", res, mo.nb, q)


@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("name", NAMES)
def test_sessions_return_the_models_bytes(gpus, programs, name, nb):
    case = mc.case(name)
    mo, hw = mc.model(case, nb), programs(name)
    chk = _checker(mo)
    planes = _run(gpus, hw, mo, chk)
    for q in range(2):
        assert planes[q] == mo.planes[q], (name, q)                                    # 1: byte-identical, both parties
    opened = _opened_witness(chk, planes, nb, case.prog.n)
    assert chk.bad == [] and chk.mod_mismatch == []                                    # 2: every opened d, e and the final planes
    v, inputs, chi = mo.opened_operands()
    single = gpus[0].r1cs_witness_synthesize(hw[0], nb, case.prog.n, 0, v, inputs, chi)
    assert tuple(opened) == tuple(single) == tuple(case.planes(nb)), name              # 3: the single-party synthesis of the opened values
    if name in GADGETS:                                                                # 4: the constraints on the finished planes
        q, circs = _circuits(gpus, case)
        try:
            rows = _residuals(gpus, circs, q, mo, chk, planes)
            assert all(x == 0 for row in rows for x in row), name
            assert chk.bad == [] and chk.mod_mismatch == []
        finally:
            for g, h in zip(gpus, circs):
                g.circuit_destroy(h)


@pytest.mark.parametrize("name", GADGETS)
def test_broken_inputs_open_to_a_nonzero_row(gpus, programs, name):
    case = mc.case(name)
    nb = 3

    def broken(p):
        v, inputs, chi = case.prover(p)
        v2, inputs2 = case.breaker(v, inputs)
        return (v2, inputs2, chi) if p == 1 else (v, inputs, chi)
    mo = mc.Model(case, nb, seed=29, which=broken)
    chk = _checker(mo)
    planes = _run(gpus, programs(name), mo, chk)
    q, circs = _circuits(gpus, case)
    try:
        rows = _residuals(gpus, circs, q, mo, chk, planes)
        assert any(rows[1]) and not any(rows[0]) and not any(rows[2]), name
        assert chk.bad == [] and chk.mod_mismatch == []
    finally:
        for g, h in zip(gpus, circs):
            g.circuit_destroy(h)


@pytest.mark.parametrize("name", ["mpc_edges", "mpc_dag70"])
def test_phase_1_then_phase_2_give_the_bytes_of_phase_0(gpus, programs, name):
    case = mc.case(name)
    prog, nb = case.prog, 3
    mo, hw = mc.model(case, nb), programs(name)
    chk = _checker(mo)
    l1 = prog.levels()[0]
    assert 0 < l1 < len(mo.rounds)
    first = _run(gpus, hw, mo, chk, phase=1, rounds=mo.rounds[:l1])                      # no challenges: they do not exist yet
    for q in range(2):
        for w in range(3):
            for pv in range(3 * nb):
                row = first[q][w][32 * pv * prog.n:32 * (pv + 1) * prog.n]
                assert row[:32 * prog.phase1] == mo.planes[q][w][32 * pv * prog.n:][:32 * prog.phase1]
                assert row[32 * prog.phase1:] == bytes(32 * (prog.n - prog.phase1))       # never given: zero
    second = _run(gpus, hw, mo, chk, phase=2, rounds=mo.rounds[l1:], planes_in=first, first_level=l1)
    for q in range(2):
        assert second[q] == mo.planes[q], (name, q)
    assert chk.bad == [] and chk.mod_mismatch == []


def test_a_phase_without_gates_has_no_rounds(gpus, programs):
    case = mc.case("mpc_edges_p2")
    mo, hw = mc.model(case, 3), programs("mpc_edges_p2")
    n = case.prog.n
    for q in range(2):
        s = gpus[q].mpc_witness_begin(hw[q], 3, 1, mo.v[q], mo.inputs[q])
        assert gpus[q].mpc_witness_levels_left(s) == 0 and gpus[q].mpc_witness_level_len(s) == 0
        assert gpus[q].mpc_witness_finish(s, 3, n) == (bytes(32 * 9 * n),) * 3
        gpus[q].mpc_witness_destroy(s)
    assert gpus[0].mpc_witness_begin(hw[0], 0, 0, None, None, mo.chi) is None             # nb == 0: no session


@pytest.mark.parametrize("name", ["shuffle4", "range_inputs8"])
def test_synthesized_planes_feed_the_two_party_commit(gpus, programs, name):
    import mpc_bulletproof_amd as m                                                       # noqa: F401
    case = mc.case(name)
    n, nb = case.prog.n, 3
    mo = mc.model(case, nb)
    chk = _checker(mo)
    planes = _run(gpus, programs(name), mo, chk)
    rnd = random.Random(404)
    d = md.Dealer(77)
    d.alpha_sh, d.alpha = mo.dealer.alpha_sh, mo.dealer.alpha
    s_L = [[rnd.randrange(N) for _ in range(n)] for _ in range(nb)]
    s_R = [[rnd.randrange(N) for _ in range(n)] for _ in range(nb)]
    bl = [[rnd.randrange(N) for _ in range(3)] for _ in range(nb)]
    sh = {key: [d.share_vec(row) for row in vals] for key, vals in (("sL", s_L), ("sR", s_R), ("bl", bl))}
    cap = 16
    gens = [g.gens_create(o.gens("G", cap), o.gens("H", cap), o.generator(), o.generator(), 8) for g in gpus]
    sess = [None, None]
    try:
        outs = []
        for q in range(2):
            ops = [md.pack([[sh[key][p][q][k] for k in range(3)] for p in range(nb)]) for key in ("sL", "sR", "bl")]
            sess[q], out = gpus[q].mpc_prover_commit(gens[q], None, nb, n, *planes[q], ops[0], ops[1], ops[2])
            outs.append(out)
        got = b"".join(chk.open_pt("%s[%d]" % (pt, p), [[outs[q][((p * 3 + k) * 3 + j) * 64:][:64] for k in range(3)] for q in range(2)])
                       for p in range(nb) for j, pt in enumerate(("A_I", "A_O", "S")))
        assert chk.bad == [] and chk.mod_mismatch == []
        opened = _opened_witness(chk, planes, nb, n)
        single, want = gpus[0].r1cs_prover_commit(gens[0], None, nb, n, *opened, md.pack(bl), s_L=md.pack(s_L), s_R=md.pack(s_R))
        gpus[0].prover_destroy(single)
        assert got == want, name
    finally:
        for q in range(2):
            if sess[q] is not None:
                gpus[q].prover_destroy(sess[q])
            gpus[q].gens_destroy(gens[q])


def test_non_canonical_limbs_are_refused_and_the_context_stays_good(gpus, programs):
    import mpc_bulletproof_amd as m
    case = mc.case("mpc_dag24")
    nb = 3
    mo, hw = mc.model(case, nb), programs("mpc_dag24")
    bad = N.to_bytes(32, "little")
    r0 = mo.rounds[0]
    G = len(r0["gates"])
    for q in range(2):
        # ... in the triples: the last scalar of the level
        s = gpus[q].mpc_witness_begin(hw[q], nb, 0, mo.v[q], mo.inputs[q], mo.chi)
        with pytest.raises(m.BpGpuError) as err:
            gpus[q].mpc_witness_mask(s, nb, r0["triples"][q][:-32] + bad)
        assert err.value.code == m.lib.E_ARG
        assert gpus[q].mpc_witness_levels_left(s) == len(mo.rounds) and gpus[q].mpc_witness_level_len(s) == G
        gpus[q].mpc_witness_destroy(s)
        # ... in the opened values: the first d
        s = gpus[q].mpc_witness_begin(hw[q], nb, 0, mo.v[q], mo.inputs[q], mo.chi)
        assert gpus[q].mpc_witness_mask(s, nb, r0["triples"][q]) == r0["masked"][q]
        with pytest.raises(m.BpGpuError) as err:
            gpus[q].mpc_witness_combine(s, bad + r0["opened"][32:])
        assert err.value.code == m.lib.E_ARG
        assert gpus[q].mpc_witness_levels_left(s) == len(mo.rounds)
        gpus[q].mpc_witness_destroy(s)
        # ... and in an operand of _begin: no session
        with pytest.raises(m.BpGpuError) as err:
            gpus[q].mpc_witness_begin(hw[q], nb, 0, bad + mo.v[q][32:], mo.inputs[q], mo.chi)
        assert err.value.code == m.lib.E_ARG
    # fresh sessions on the same contexts give the right bytes
    chk = _checker(mo)
    planes = _run(gpus, hw, mo, chk)
    assert planes[0] == mo.planes[0] and planes[1] == mo.planes[1]
    assert chk.bad == [] and chk.mod_mismatch == []
