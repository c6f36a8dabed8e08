"""bpgpu_r1cs_prove_values / _dev and the pool forms (bpgpu_pool_circuit_create_param, bpgpu_pool_witness_*,
bpgpu_pool_r1cs_prove_values) on the CPU: exported, bound and declared for Rust with the header's argument counts; every refusal that
precedes a launch comes back before a device is touched (hand-made headers stand in for the handles, a zeroed block for the context);
the pool call refuses handles of another pool and answers nb == 0 with BPGPU_OK.  No GPU needed."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name -> number of arguments
NEW = {"bpgpu_r1cs_prove_values": 28, "bpgpu_r1cs_prove_values_dev": 28,      # ctx g c w nb | 9 operands | 14 results
       "bpgpu_pool_circuit_create_param": 10, "bpgpu_pool_witness_create": 12, "bpgpu_pool_witness_destroy": 2, "bpgpu_pool_witness_get": 2,
       "bpgpu_pool_r1cs_prove_values": 28}


def _lib():
    import mpc_bulletproof_amd as m
    return m, m.lib._lib


def test_entry_points_are_exported_bound_and_declared_with_their_argument_counts():
    m, lib = _lib()
    from mpc_bulletproof_amd._abi import PROTOS
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "bpgpu.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    raw = C.CDLL(m.lib.SO_PATH)
    for name, nargs in NEW.items():
        assert hasattr(raw, name), name
        assert name in m.lib.SYMBOLS, name
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        rdecl = re.search(r"pub fn %s\(([^;]*?)\)( -> [^;]+)?;" % name, rs, re.S)
        assert rdecl and len([a for a in rdecl.group(1).split(",") if a.strip()]) == nargs, name
        assert len(PROTOS[name][1]) == nargs and getattr(lib, name).argtypes == PROTOS[name][1], name
    assert "pub struct bpgpu_pool_witness {" in rs
    assert lib.bpgpu_pool_witness_destroy.restype is None and lib.bpgpu_pool_witness_get.restype is C.c_void_p
    assert callable(m.BpGpu.r1cs_prove_values)
    for method in ("circuit_create_param", "witness_create", "witness_destroy", "witness_get", "r1cs_prove_values"):
        assert callable(getattr(m.BpPool, method)), method
    assert m.lib.ProveValues._fields == ("ok", "first_bad_row", "first_bad_gate", "V", "V_compressed", "points", "scalars", "wire", "challenges",
                                         "states", "chi", "planes")
    # no numbered option and no profiling kind was added
    full = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    assert "#define BPGPU_PROF_KINDS 24" in full


def test_header_documents_the_calls():
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    block = " ".join(hdr[hdr.index("Prove from COMMITTED VALUES in one call"):hdr.index("int bpgpu_r1cs_prove_values(")].replace("*", " ").split())
    for phrase in ("ONE-PHASE", "TWO-PHASE", "necessarily runs AFTER the proof", "REJECTED PROVERS SHIP NOTHING", "kind 22", "zero bytes",
                   "version byte 0", "never waits for ok", "byte for byte", "BPGPU_OPT_WITNESS_ROUTE", "nchi > 1", "bpgpu_set_shard(world > 1)",
                   "BPGPU_E_LEN for n == 0", "BPGPU_E_GENS", "nb == 0: BPGPU_OK", "bpgpu_input_flag", "no session and no pool memory",
                   "profiles/prove_values.log", "UNMEASURED"):
        assert phrase in block, phrase
    pool = " ".join(hdr[hdr.index("---- pools:"):hdr.index("#define BPGPU_POOL_MAX_SLOTS")].replace("*", " ").split())
    for phrase in ("bpgpu_pool_circuit_create_param", "bpgpu_pool_witness_create", "bpgpu_pool_r1cs_prove_values", "refuse such a handle"):
        assert phrase in pool, phrase
    assert "a pool serves circuits without randomized constraints only" not in pool


# ctx g c w nb | init label v v_blinding inputs s_L s_R keys blindings | V Vc ok row gate points scalars wire ch states chi | a_L a_R a_O
def _good(two):
    fake_ctx = (C.c_uint8 * (1 << 16))()
    gens = (C.c_size_t * 64)(4)                                   # bpgpu_gens: capacity first
    circ = (C.c_size_t * 64)(5, 3, 2, 7, 1 if two else 0)         # bpgpu_circuit: q, n, m, nnz, nchi
    prog = (C.c_size_t * 64)(3, 1 if two else 3, 2, 1 if two else 0, 1)      # bpgpu_witness: n, n1, m, nchi, INPUT pairs
    buf = (C.c_uint8 * 4096)()
    return [fake_ctx, gens, circ, prog, 1, buf, buf if two else None, buf, buf, buf, buf, buf, None, buf,
            None, None, buf, None, None, buf, buf, None, None, None, None, None, None, None], buf


def test_refusals_come_back_without_a_device():
    m, lib = _lib()
    E, EL, EG = m.lib.E_ARG, m.lib.E_LEN, m.lib.E_GENS
    hdr = lambda *xs: (C.c_size_t * 64)(*xs)     # noqa: E731
    for name in ("bpgpu_r1cs_prove_values", "bpgpu_r1cs_prove_values_dev"):
        fn = getattr(lib, name)
        for two in (False, True):
            good, buf = _good(two)

            def rc(**kw):
                a = list(good)
                for k, v in kw.items():
                    a[int(k[1:])] = v
                return fn(*a)
            if lib.bpgpu_device_count() == 0:
                assert rc() == m.lib.E_DEVICE, name           # past the refusals the call selects the context's device
            for hole in (0, 1, 2, 3):                                            # context, generators, circuit, program
                assert rc(**{"a%d" % hole: None}) == E, (name, hole)
            for hole in (5, 7, 8, 9, 13, 16, 19, 20):         # init_states, v, v_blinding, inputs, blindings, ok, points, scalars
                assert rc(**{"a%d" % hole: None}) == E, (name, two, hole)
            assert rc(a6=None if two else buf) == E, (name, two)                 # a label missing | given to a one-phase pair
            assert rc(a10=None) == E and rc(a11=None) == E                       # one of s_L, s_R
            assert rc(a12=buf) == E and rc(a10=None, a11=None) == E              # both sources, or neither
            assert rc(a25=buf) == E and rc(a25=buf, a26=buf) == E and rc(a26=buf, a27=buf) == E     # some of the witness planes
            n1, nchi = (1, 1) if two else (3, 0)
            for bad in ((4, n1, 2, nchi, 1), (3, n1, 3, nchi, 1), (3, n1, 2, 1 - nchi, 1)):          # not the circuit's n, m, nchi
                assert rc(a3=hdr(*bad)) == E, (name, two, bad)
            assert rc(a2=hdr(5, 3, 2, 7, 2), a3=hdr(3, 1, 2, 2, 1)) == E, name                       # nchi > 1
            assert rc(a1=hdr(2)) == EG, name                                                          # padded n above the capacity
            if two:
                assert rc(a3=hdr(3, 3, 2, 1, 1)) == EL, name                                          # n1 >= n: no second phase
                assert rc(a2=hdr(5, 0, 2, 7, 1), a3=hdr(0, 0, 2, 1, 0)) == EL, name                   # n == 0
            else:
                assert rc(a3=hdr(3, 2, 2, 0, 1)) == E, name                                           # a one-phase program has n1 == n
                assert rc(a2=hdr(5, 0, 2, 7, 0), a3=hdr(0, 0, 2, 0, 0)) == EL, name                   # n == 0
            assert rc(a2=hdr(5, 3, 1 << 31, 7, nchi), a3=hdr(3, n1, 1 << 31, nchi, 1)) == EL, name    # nb m above 2^30 commitments
            # a context after bpgpu_set_shard(world > 1) -- the call stores two words in the context and needs no device
            assert lib.bpgpu_set_shard(good[0], 0, 2) == 0 and rc() == E, (name, two)
            assert lib.bpgpu_set_shard(good[0], 0, 1) == 0
            if lib.bpgpu_device_count() == 0:
                assert rc() == m.lib.E_DEVICE, name
            # nb == 0: nothing to do, nothing touched
            a = good[:4] + [0] + [None] * 23
            assert fn(*a) == 0, name
            # optional results given: still past the refusals
            if lib.bpgpu_device_count() == 0:
                assert rc(a14=buf, a15=buf, a17=buf, a18=buf, a21=buf, a22=buf, a23=buf, a24=buf, a25=buf, a26=buf, a27=buf) == m.lib.E_DEVICE


def test_null_handles_are_refused_by_the_pool_forms_without_a_crash():
    m, lib = _lib()
    E = m.lib.E_ARG
    buf = (C.c_uint8 * 4096)()
    out = C.c_void_p(0xdead)
    assert lib.bpgpu_pool_circuit_create_param(None, 1, 1, buf, buf, buf, buf, 2, 1, C.byref(out)) == E and not out.value
    out = C.c_void_p(0xdead)
    assert lib.bpgpu_pool_witness_create(None, 2, 1, 1, 1, buf, buf, buf, buf, buf, buf, C.byref(out)) == E and not out.value
    assert lib.bpgpu_pool_witness_create(buf, 2, 1, 1, 1, buf, buf, buf, buf, buf, buf, None) == E
    assert lib.bpgpu_pool_witness_get(None, 0) is None
    lib.bpgpu_pool_witness_destroy(None, None)
    assert lib.bpgpu_pool_r1cs_prove_values(None, buf, buf, buf, 1, *([buf] * 23)) == E
    assert lib.bpgpu_pool_r1cs_prove_values(None, None, None, None, 0, *([None] * 23)) == E


def test_pool_call_with_handles_of_another_pool_and_with_no_provers():
    """a pool handle's first word is its pool: hand-made headers suffice, and neither answer needs a device or wakes a worker"""
    m, lib = _lib()
    E = m.lib.E_ARG
    pool, other = (C.c_uint8 * 4096)(), (C.c_uint8 * 4096)()
    mine = lambda: (C.c_size_t * 64)(C.addressof(pool))          # noqa: E731
    theirs = lambda: (C.c_size_t * 64)(C.addressof(other))       # noqa: E731
    buf = (C.c_uint8 * 4096)()
    ops = [buf] * 23
    for g, c, w in ((theirs(), mine(), mine()), (mine(), theirs(), mine()), (mine(), mine(), theirs()), (None, mine(), mine()),
                    (mine(), None, mine()), (mine(), mine(), None)):
        assert lib.bpgpu_pool_r1cs_prove_values(pool, g, c, w, 1, *ops) == E
        assert lib.bpgpu_pool_r1cs_prove_values(pool, g, c, w, 0, *ops) == E
    assert lib.bpgpu_pool_r1cs_prove_values(pool, mine(), mine(), mine(), 0, *([None] * 23)) == 0      # nb == 0: BPGPU_OK, nothing touched
    assert bytes(buf) == bytes(4096)
    # a parametric pool circuit (nchi, behind the pool, the per-slot handles and n, m) is refused by the calls that take numeric ones
    param = (C.c_size_t * 64)(C.addressof(pool), 0, 0, 0, 3, 2, 1)
    assert lib.bpgpu_pool_r1cs_prove_fs(pool, mine(), param, 1, *([buf] * 14)) == E
    assert lib.bpgpu_pool_r1cs_verify_stream(pool, mine(), param, 1, 0, 2, buf, buf, buf, buf, None) == E
    assert lib.bpgpu_pool_r1cs_verify_screened(pool, mine(), param, 1, 0, 2, buf, buf, buf, buf, buf, None) == E
    assert lib.bpgpu_pool_r1cs_verify_combined(pool, mine(), param, 1, 0, 2, buf, buf, buf, buf, buf) == E
