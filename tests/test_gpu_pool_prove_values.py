"""bpgpu_pool_r1cs_prove_values: the one call dealt over the slots of a pool ({0, 0} and {0, 0, 0} on the one GPU: at most three
contexts, one process) against the single-context call on the whole queue, which tests/test_gpu_prove_values.py holds against the
chain of existing calls.  One one-phase and one two-phase case, nb = 5 (shares 3 + 2 | 2 + 2 + 1) and nb = 1 (empty slots), a rejected
prover in the last non-empty share, and the refusal of a parametric pool circuit by the calls that have no use for one."""
import pytest

import oracle_lib as o
import prove_values_cases as pc

pytestmark = pytest.mark.gpu
NAMES = ("range8x2", "shuffle4")


@pytest.fixture(scope="module", params=(2, 3), ids=("two-slots", "three-slots"))
def pool(request):
    import mpc_bulletproof_amd as m
    p = m.BpPool([0] * request.param)
    gens = p.gens_create(o.gens("G", pc.CAP), o.gens("H", pc.CAP), o.generator(), o.generator(), 8)
    made = {name: pc.handles(p, name) for name in NAMES}
    yield p, gens, made
    for circ, w in made.values():
        p.witness_destroy(w)
        p.circuit_destroy(circ)
    p.gens_destroy(gens)
    p.close()


def single(pool, gens, made, name, nb, ops):
    """the single-context call on slot 0's borrowed context and handles"""
    prog = pc.case(name).prog
    circ, w = made[name]
    g = pool.ctx(0)
    return g.r1cs_prove_values(pool.gens_get(gens, 0), pool.circuit_get(circ, 0), pool.witness_get(w, 0), nb, prog.n, prog.m,
                               want_witness=True, **ops)


@pytest.mark.parametrize("nb,bad", ((5, None), (1, None), (5, 4)), ids=("five", "one", "rejected-last-share"))
@pytest.mark.parametrize("keys", (False, True), ids=("explicit", "keys"))
@pytest.mark.parametrize("name", NAMES)
def test_pool_equals_the_single_context_call(pool, name, keys, nb, bad):
    p, gens, made = pool
    prog = pc.case(name).prog
    circ, w = made[name]
    lo = p.shares(nb, p.slots(), 1)
    if bad is not None:
        last = max(s for s in range(p.slots()) if lo[s + 1] > lo[s])
        assert last > 0 and lo[last] <= bad < lo[last + 1]
    ops = pc.operands(name, nb, keys, bad=bad)
    want = single(p, gens, made, name, nb, ops)
    got = p.r1cs_prove_values(gens, circ, w, nb, prog.n, prog.m, want_witness=True, **ops)
    for field, a, b in zip(pc.FIELDS, got, want):
        assert a == b, field
    assert got.ok == [int(q != bad) for q in range(nb)]
    if bad is not None:
        for field in ("points", "scalars", "wire", "challenges", "states"):
            assert pc.rows(name, field, getattr(got, field), [bad]) == bytes(pc.row_bytes(name)[field]), field


def test_parametric_pool_circuit_is_refused_by_the_other_calls(pool):
    import ctypes as C
    import mpc_bulletproof_amd as m
    p, gens, made = pool
    circ, _ = made["shuffle4"]
    buf = (C.c_uint8 * 4096)()
    lib = m.lib._lib
    assert lib.bpgpu_pool_r1cs_prove_fs(p.pool, gens, circ, 1, *([buf] * 14)) == m.lib.E_ARG
    assert lib.bpgpu_pool_r1cs_verify_stream(p.pool, gens, circ, 1, 0, 3, buf, buf, buf, buf, None) == m.lib.E_ARG
    assert lib.bpgpu_pool_r1cs_verify_stream(p.pool, gens, circ, 0, 0, 3, None, None, None, None, None) == m.lib.E_ARG
    # handles of another kind of call are refused before a worker is woken, and the pool proves afterwards
    numeric, _ = made["range8x2"]
    prog = pc.case("shuffle4").prog
    with pytest.raises(m.BpGpuError) as e:
        p.r1cs_prove_values(gens, numeric, made["shuffle4"][1], 1, prog.n, prog.m, **pc.operands("shuffle4", 1, True))
    assert e.value.code == m.lib.E_ARG and "before any slot was woken" in lib.bpgpu_pool_last_error(p.pool).decode()
