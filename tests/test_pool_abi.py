"""The pool entry points (include/bpgpu.h, bpgpu_pool_*) on the CPU: exported, bound and declared for Rust; the refusals that need no
device; and the split every pool call uses (bpgpu_pool_shares), which needs none either.  No GPU needed."""
import ctypes as C
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"bpgpu_pool_create": 3, "bpgpu_pool_destroy": 1, "bpgpu_pool_slots": 1, "bpgpu_pool_device": 2, "bpgpu_pool_ctx": 2,
       "bpgpu_pool_set_option": 3, "bpgpu_pool_last_error": 1, "bpgpu_pool_gens_create": 8, "bpgpu_pool_gens_destroy": 2,
       "bpgpu_pool_gens_get": 2, "bpgpu_pool_circuit_create": 9, "bpgpu_pool_circuit_create_ark": 9, "bpgpu_pool_circuit_destroy": 2,
       "bpgpu_pool_circuit_get": 2, "bpgpu_pool_shares": 4, "bpgpu_pool_r1cs_verify_stream": 11, "bpgpu_pool_r1cs_verify_screened": 12,
       "bpgpu_pool_r1cs_verify_combined": 11, "bpgpu_pool_r1cs_prove_fs": 18}


def _m():
    import mpc_bulletproof_amd as m
    return m, m.lib._lib


def test_entry_points_are_exported_bound_and_declared_with_their_argument_counts():
    m, lib = _m()
    from mpc_bulletproof_amd._abi import PROTOS
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "bpgpu.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "shim", "src", "sys.rs")).read()
    raw = C.CDLL(m.lib.SO_PATH)
    for name, nargs in NEW.items():
        assert hasattr(raw, name), name
        assert name in m.lib.SYMBOLS, name
        restype, argtypes = PROTOS[name]
        assert len(argtypes) == nargs, name
        fn = getattr(lib, name)
        assert fn.restype is restype and fn.argtypes == argtypes, name
        decl = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, re.S)
        assert decl and len(decl.group(1).split(",")) == nargs, name
        rdecl = re.search(r"pub fn %s\(([^;]*?)\)( -> [^;]+)?;" % name, rs, re.S)
        assert rdecl and len([a for a in rdecl.group(1).split(",") if a.strip()]) == nargs, name
    for t in ("bpgpu_pool", "bpgpu_pool_gens", "bpgpu_pool_circuit"):
        assert "pub struct %s {" % t in rs, t
    assert "pub const BPGPU_POOL_MAX_SLOTS: c_int = 32;" in rs and m.lib.POOL_MAX_SLOTS == 32
    assert lib.bpgpu_pool_slots.restype is C.c_size_t and lib.bpgpu_pool_ctx.restype is C.c_void_p
    assert lib.bpgpu_pool_last_error.restype is C.c_char_p and lib.bpgpu_pool_destroy.restype is None
    for method in ("set_option", "gens_create", "gens_destroy", "gens_get", "circuit_create", "circuit_destroy", "circuit_get", "shares",
                   "ctx", "device", "slots", "close", "r1cs_verify_stream", "r1cs_verify_screened", "r1cs_verify_combined", "r1cs_prove_fs"):
        assert callable(getattr(m.BpPool, method)), method


def test_header_documents_the_pool():
    hdr = open(os.path.join(ROOT, "include", "bpgpu.h")).read()
    block = " ".join(hdr[hdr.index("---- pools:"):hdr.index("#define BPGPU_POOL_MAX_SLOTS")].replace("*", " ").split())
    for phrase in ("one persistent host thread", "once per DISTINCT device", "all or nothing", "Parametric circuits", "no pool form",
                   "LOWEST failing slot", "before any worker is woken", "nb == 0 returns BPGPU_OK and touches nothing", "UNMEASURED",
                   "the first and the last byte", "staged copies", "bpgpu_points_sum on slot 0", "never depends on timing or data",
                   "one pool per calling thread", "stays with bpgpu_set_shard"):
        assert phrase in block, phrase


def test_pool_create_refusals():
    """BPGPU_E_ARG for a null out, a null list, no slot and 33 slots, on any machine; without a device a valid list gives
    BPGPU_E_DEVICE (and with one, an index past the last device does)"""
    m, lib = _m()
    E, D = m.lib.E_ARG, m.lib.E_DEVICE
    one, many = (C.c_int * 1)(0), (C.c_int * 33)()
    out = C.c_void_p(0xdead)
    assert lib.bpgpu_pool_create(one, 1, None) == E
    assert lib.bpgpu_pool_create(None, 1, C.byref(out)) == E and not out.value
    assert lib.bpgpu_pool_create(one, 0, C.byref(out)) == E and not out.value
    assert lib.bpgpu_pool_create(many, 33, C.byref(out)) == E and not out.value
    count = lib.bpgpu_device_count()
    if count == 0:
        assert lib.bpgpu_pool_create(one, 1, C.byref(out)) == D and not out.value
        assert lib.bpgpu_pool_create(many, 32, C.byref(out)) == D and not out.value
        assert lib.bpgpu_pool_create((C.c_int * 2)(0, 0), 2, C.byref(out)) == D and not out.value
        with pytest.raises(m.BpGpuError) as e:
            m.BpPool([0, 0])
        assert e.value.code == D
    assert lib.bpgpu_pool_create((C.c_int * 2)(0, count), 2, C.byref(out)) == D and not out.value
    assert lib.bpgpu_pool_create((C.c_int * 1)(-1), 1, C.byref(out)) == D and not out.value


def test_a_null_pool_is_refused_everywhere_without_a_crash():
    m, lib = _m()
    E = m.lib.E_ARG
    buf = (C.c_uint8 * 4096)()
    out = C.c_void_p(0xdead)
    n, z = 4, 0
    assert lib.bpgpu_pool_set_option(None, m.lib.OPT["stream_batch"], 16) == E
    assert lib.bpgpu_pool_gens_create(None, buf, buf, 4, buf, buf, 8, C.byref(out)) == E and not out.value
    out = C.c_void_p(0xdead)
    assert lib.bpgpu_pool_circuit_create(None, 1, buf, buf, buf, buf, 2, 1, C.byref(out)) == E and not out.value
    out = C.c_void_p(0xdead)
    assert lib.bpgpu_pool_circuit_create_ark(None, 1, buf, buf, buf, buf, 2, 1, C.byref(out)) == E and not out.value
    nf = C.c_size_t(0)
    assert lib.bpgpu_pool_r1cs_verify_stream(None, buf, buf, n, z, z, buf, buf, buf, buf, None) == E
    assert lib.bpgpu_pool_r1cs_verify_stream(None, None, None, z, z, z, None, None, None, None, None) == E
    assert lib.bpgpu_pool_r1cs_verify_screened(None, buf, buf, n, z, z, buf, buf, buf, buf, buf, C.byref(nf)) == E
    assert lib.bpgpu_pool_r1cs_verify_combined(None, buf, buf, n, z, z, buf, buf, buf, buf, buf) == E
    assert lib.bpgpu_pool_r1cs_prove_fs(None, buf, buf, n, *([buf] * 14)) == E
    assert lib.bpgpu_pool_r1cs_prove_fs(None, None, None, z, *([None] * 14)) == E
    # the entry points without a status: nothing to report, nothing to crash on
    assert lib.bpgpu_pool_slots(None) == 0
    assert lib.bpgpu_pool_device(None, 0) == E
    assert lib.bpgpu_pool_ctx(None, 0) is None
    assert lib.bpgpu_pool_last_error(None) == b""
    assert lib.bpgpu_pool_gens_get(None, 0) is None and lib.bpgpu_pool_circuit_get(None, 0) is None
    lib.bpgpu_pool_gens_destroy(None, None)
    lib.bpgpu_pool_circuit_destroy(None, None)
    lib.bpgpu_pool_destroy(None)


NBS = (0, 1, 15, 16, 17, 150, 2560 * 3 + 1)
NSLOTS = (1, 2, 3, 8, 32)
GRANULES = (1, 16, 2560)


@pytest.mark.parametrize("nb,nslots,granule", list(itertools.product(NBS, NSLOTS, GRANULES)))
def test_shares(nb, nslots, granule):
    m, _ = _m()
    lo = m.lib.pool_shares(nb, nslots, granule)
    assert len(lo) == nslots + 1 and lo[0] == 0 and lo[nslots] == nb
    assert all(a <= b for a, b in zip(lo, lo[1:]))
    size = [b - a for a, b in zip(lo, lo[1:])]
    nonempty = [s for s in range(nslots) if size[s]]
    for s in nonempty[:-1]:                                  # every share but the last non-empty one: whole granules
        assert size[s] % granule == 0, (s, size)
    granules = [-(-x // granule) for x in size]
    assert sum(granules) == -(-nb // granule)
    assert max(granules) - min(granules) <= 1 and all(a >= b for a, b in zip(granules, granules[1:])), granules
    if nonempty:                                             # the slots past the last granule are empty, and only they
        assert nonempty == list(range(len(nonempty)))
    assert m.BpPool.shares(nb, nslots, granule) == lo


def test_shares_of_the_gpu_tests_queue():
    """150 proofs in batches of 16 over three slots: 4 + 3 + 3 batches"""
    m, _ = _m()
    assert m.lib.pool_shares(150, 3, 16) == [0, 64, 112, 150]
    assert m.lib.pool_shares(150, 2, 16) == [0, 80, 150]
    assert m.lib.pool_shares(5, 3, 16) == [0, 5, 5, 5]
    assert m.lib.pool_shares(7, 3, 1) == [0, 3, 5, 7]


def test_shares_refusals():
    m, lib = _m()
    lo = (C.c_size_t * 4)(7, 7, 7, 7)
    assert lib.bpgpu_pool_shares(10, 0, 1, lo) == m.lib.E_ARG
    assert lib.bpgpu_pool_shares(10, 3, 0, lo) == m.lib.E_ARG
    assert lib.bpgpu_pool_shares(10, 3, 1, None) == m.lib.E_ARG
    assert list(lo) == [7, 7, 7, 7]
    for bad in ((10, 0, 1), (10, 3, 0)):
        with pytest.raises(m.BpGpuError):
            m.lib.pool_shares(*bad)
