"""ctypes binding of libbpgpu.so (include/bpgpu.h).  Byte-level, no torch types."""
import collections
import ctypes as C
import os

from ._abi import PROTOS

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.path.join(_HERE, "libbpgpu.so")

SYMBOLS = sorted(PROTOS)     # every entry point of include/bpgpu.h (_abi.py is generated from it by tools/gen_rust_sys.py)

MIXED_MAX_GROUPS = 64       # BPGPU_MIXED_MAX_GROUPS
MIXED_MAX_SEGMENTS = 16     # BPGPU_MIXED_MAX_SEGMENTS


class VerifyGroup(C.Structure):
    """bpgpu_verify_group: one circuit's run of proofs in a mixed verification call (include/bpgpu.h)"""
    _fields_ = [("circuit", C.c_void_p), ("nb", C.c_size_t), ("n1", C.c_size_t), ("k", C.c_size_t),
                ("points", C.c_void_p), ("scalars", C.c_void_p), ("challenges", C.c_void_p),
                ("gadget_challenges", C.c_void_p), ("rho", C.c_void_p), ("ok", C.c_void_p)]


class WireGroup(C.Structure):
    """bpgpu_wire_group: one circuit's run of wire-format proofs in a mixed verification call (include/bpgpu.h)"""
    _fields_ = [("circuit", C.c_void_p), ("nb", C.c_size_t), ("n1", C.c_size_t), ("proof_len", C.c_size_t),
                ("proofs", C.c_void_p), ("commitments", C.c_void_p), ("init_states", C.c_void_p),
                ("gadget_label", C.c_void_p), ("rho", C.c_void_p), ("ok", C.c_void_p)]


class BpGpuError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        super().__init__(f"bpgpu error {code}: {what}")


def load():
    if not os.path.exists(SO_PATH):
        raise ImportError(
            f"{SO_PATH} is missing: the HIP extension has not been built "
            "(run __graft_entry__.build()).  There is no CPU fallback.")
    lib = C.CDLL(SO_PATH)
    for name, (restype, argtypes) in PROTOS.items():     # an integer of the wrong width is refused, never truncated
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


_lib = load()


def host_alloc(nbytes, data=None):
    """page-locked staging memory (bpgpu_host_alloc), optionally filled with `data`; returns a c_void_p"""
    p = C.c_void_p()
    rc = _lib.bpgpu_host_alloc(nbytes, C.byref(p))
    if rc or not p.value:
        raise BpGpuError(rc or E_OOM, "bpgpu_host_alloc")
    if data is not None:
        C.memmove(p, data if isinstance(data, bytes) else bytes(data), len(data))
    return p


def host_free(p):
    _lib.bpgpu_host_free(p)


E_ARG, E_LEN, E_DEVICE, E_OOM, E_GENS = -1, -2, -3, -4, -5
# bpgpu_set_option (include/bpgpu.h BPGPU_OPT_*)
OPT = {"msm_wp_max": 1, "msm_pip2_single": 2, "verify_no_fuse": 3, "verify_window_parallel": 4, "verify_straus_np": 5,
       "ipp_literal": 6, "vs_large_min": 7, "table_np": 8, "ipp_table_max_n": 9, "stream_lanes": 10, "stream_batch": 11, "screen_batch": 12,
       "horner_form": 13, "horner_row_max": 14, "pippenger_min": 15, "ipp_pippenger_min": 16, "fixed_lpm": 17, "groups_form": 18, "fixed_chunk_gens": 19,
       "witness_route": 20, "witness_scan_min": 21}
# bpgpu_profile_read kinds (include/bpgpu.h BPGPU_PROF_KINDS)
PROF_NAMES = ["verify_scalars", "fixed_msm", "points_from_boundary", "straus", "verify_finalize", "transcript", "verify_msm",
              "verify_windows", "verify_front", "verify_groups", "verify_back", "verify_verdict", "combined_front_scalars_digits",
              "combined_sort_accum_reduce", "combined_unused", "combined_final", "prover_commit", "prover_polys", "msm_gens", "ipp_begin",
              "ipp_rounds", "ipp_round_msm", "prove_fs_links", "wire_decode"]
PROF_KINDS = len(PROF_NAMES)


def _buf(b):
    """a read-only operand for the C ABI WITHOUT copying it: the address of the bytes object's own storage (kept alive by the
    caller's reference for the duration of the call).  Copying 100 MB of operands twice on the Python side was what made a 2^20-term
    bpgpu_msm from "host buffers" look 15x slower than the resident call."""
    if not isinstance(b, bytes):
        b = bytes(b)
    return C.c_char_p(b if len(b) else b"\0")


def _inout(b):
    """an IN/OUT operand (bpgpu_batch_inverse inverts in place): a private, writable copy"""
    b = bytes(b)
    return (C.c_uint8 * max(len(b), 1)).from_buffer_copy(b if len(b) else b"\0")


def _out(n):
    return (C.c_uint8 * max(n, 1))()


def device_count():
    return _lib.bpgpu_device_count()


def hw_queues():
    """-> (inherited, in_force): GPU_MAX_HW_QUEUES as the process environment held it when libbpgpu.so was loaded and as the library
    left it (bpgpu_hw_queues: -1 unset, -2 not a number).  os.environ is a snapshot that does not see the library's setenv."""
    inherited, in_force = C.c_int(0), C.c_int(0)
    rc = _lib.bpgpu_hw_queues(C.byref(inherited), C.byref(in_force))
    if rc:
        raise BpGpuError(rc, _lib.bpgpu_strerror(rc).decode())
    return inherited.value, in_force.value


# bpgpu_pippenger_plan (include/bpgpu.h BPGPU_PIP_PLAN_*)
PIP_PLAN_FIELDS = ("c", "W", "two_level", "task", "task_search", "task_sort", "scan", "coarse_scan", "final_quad", "chunks")


def pippenger_plan(nb, n):
    """the launch route of the bucket-method MSM for nb instances of n terms, as a dict over PIP_PLAN_FIELDS (needs no device)"""
    out = (C.c_int32 * len(PIP_PLAN_FIELDS))()
    rc = _lib.bpgpu_pippenger_plan(nb, n, out)
    if rc:
        raise BpGpuError(rc, _lib.bpgpu_strerror(rc).decode())
    return dict(zip(PIP_PLAN_FIELDS, out))


# bpgpu_witness_plan (include/bpgpu.h BPGPU_WIT_PLAN_*); gate ops BPGPU_GATE_*
WIT_PLAN_FIELDS = ("levels1", "levels2", "widest", "long_rows", "inputs", "route1", "route2")
GATE_MUL, GATE_INPUT, GATE_BIT = 0, 1, 2
GATE_INV = 4         # (3 is no op: include/bpgpu.h)
GATE_DIVREM = 6      # (and neither is 5)


def _u32s(xs, pad=1):
    return (C.c_uint32 * max(len(xs), pad))(*xs)


def _label(gadget_label):
    """a gadget label zero-padded to 32 bytes, or None (a circuit with attached labels, circuit_set_gadget_labels)"""
    return None if gadget_label is None else _buf((bytes(gadget_label) + bytes(32))[:32])


def witness_plan(n, n1, nchi, op, row_ptr, kind, idx, nb):
    """the dependency levels of a gate program and the launch form of each phase for nb provers, as a dict over WIT_PLAN_FIELDS
    (needs no device)"""
    out = (C.c_int32 * len(WIT_PLAN_FIELDS))()
    rc = _lib.bpgpu_witness_plan(n, n1, nchi, _buf(bytes(op)), _u32s(row_ptr), _u32s(kind), _u32s(idx), nb, out)
    if rc:
        raise BpGpuError(rc, _lib.bpgpu_strerror(rc).decode())
    return dict(zip(WIT_PLAN_FIELDS, out))


# bpgpu_witness_chains (include/bpgpu.h BPGPU_WIT_CHAIN_*)
WIT_CHAIN_FIELDS = ("chains1", "chains2", "members1", "members2", "longest1", "longest2", "levels1", "levels2")


def witness_chains(n, n1, nchi, op, row_ptr, kind, idx):
    """the product chains of a gate program -- per phase their number, their members, the longest and the compressed levels -- as a
    dict over WIT_CHAIN_FIELDS (needs no device)"""
    out = (C.c_int32 * len(WIT_CHAIN_FIELDS))()
    rc = _lib.bpgpu_witness_chains(n, n1, nchi, _buf(bytes(op)), _u32s(row_ptr), _u32s(kind), _u32s(idx), out)
    if rc:
        raise BpGpuError(rc, _lib.bpgpu_strerror(rc).decode())
    return dict(zip(WIT_CHAIN_FIELDS, out))


# bpgpu_witness_affine_chains (include/bpgpu.h BPGPU_WIT_AFF_*)
WIT_AFF_FIELDS = ("chains1", "chains2", "members1", "members2", "affine1", "affine2", "longest1", "longest2", "levels1", "levels2")


def witness_affine_chains(n, n1, nchi, op, row_ptr, kind, idx):
    """the extended chains of a gate program, product and affine members together -- per phase their number, all their members, the
    affine ones among them, the longest and the extended compressed levels -- as a dict over WIT_AFF_FIELDS (needs no device)"""
    out = (C.c_int32 * len(WIT_AFF_FIELDS))()
    rc = _lib.bpgpu_witness_affine_chains(n, n1, nchi, _buf(bytes(op)), _u32s(row_ptr), _u32s(kind), _u32s(idx), out)
    if rc:
        raise BpGpuError(rc, _lib.bpgpu_strerror(rc).decode())
    return dict(zip(WIT_AFF_FIELDS, out))


def witness_gate_levels(n, n1, nchi, op, row_ptr, kind, idx):
    """the dependency level of every gate of a program inside its phase (bpgpu_witness_gate_levels): slot t of a round of the
    two-party witness sessions is the t-th gate of that level in ascending gate index (needs no device)"""
    out = (C.c_uint32 * max(n, 1))()
    rc = _lib.bpgpu_witness_gate_levels(n, n1, nchi, _buf(bytes(op)), _u32s(row_ptr), _u32s(kind), _u32s(idx), out)
    if rc:
        raise BpGpuError(rc, _lib.bpgpu_strerror(rc).decode())
    return list(out)[:n]


ProveValues = collections.namedtuple("ProveValues", "ok first_bad_row first_bad_gate V V_compressed points scalars wire challenges states "
                                                    "chi planes")


def _prove_values_host(call, nb, n, m, lab, init_states, v, v_blinding, inputs, s_L, s_R, vector_keys, blindings, want_wire, want_witness,
                       nchi=None):
    """the host form's buffers around `call(nb, operands..., results...)`: bpgpu_r1cs_prove_values, or the pool's -> ProveValues (chi
    None for a one-phase circuit, wire and planes None unless asked for).  nchi: the circuit's gadget challenges (None: one with a label,
    none without)"""
    nchi = (1 if lab is not None else 0) if nchi is None else nchi
    two = nchi != 0
    k = max(n - 1, 0).bit_length()
    nvar, plen = 11 + 2 * k, 1 + (14 if two else 11) * 32 + (2 * k + 2) * 32
    ok, row, gate = (C.c_int32 * max(nb, 1))(), (C.c_int64 * max(nb, 1))(), (C.c_int64 * max(nb, 1))()
    V, Vc = _out(64 * nb * m), _out(32 * nb * m)
    pts, sc, ch, so = _out(64 * nb * nvar), _out(160 * nb), _out(32 * nb * (5 + k)), _out(32 * nb)
    chi = _out(32 * nb * nchi) if two else None
    wire = _out(nb * plen) if want_wire else None
    planes = [_out(32 * nb * n) if want_witness else None for _ in range(3)]
    opt = lambda b: b if b is None or isinstance(b, C.c_void_p) else _buf(b)     # noqa: E731
    call(nb, opt(init_states), lab, opt(v), opt(v_blinding), opt(inputs), opt(s_L), opt(s_R), opt(vector_keys), opt(blindings), V, Vc, ok, row,
         gate, pts, sc, wire, ch, so, chi, *planes)
    return ProveValues(list(ok)[:nb], list(row)[:nb], list(gate)[:nb], bytes(V)[:64 * nb * m], bytes(Vc)[:32 * nb * m],
                       bytes(pts)[:64 * nb * nvar], bytes(sc)[:160 * nb], bytes(wire)[:nb * plen] if want_wire else None,
                       bytes(ch)[:32 * nb * (5 + k)], bytes(so)[:32 * nb], bytes(chi)[:32 * nb * nchi] if two else None,
                       tuple(bytes(p)[:32 * nb * n] for p in planes) if want_witness else None)


class BpGpu:
    """One context on one device.  All byte encodings as in include/bpgpu.h."""

    witness_plan = staticmethod(witness_plan)
    witness_chains = staticmethod(witness_chains)
    witness_affine_chains = staticmethod(witness_affine_chains)

    def __init__(self, device=0):
        self.ctx = C.c_void_p()
        rc = _lib.bpgpu_create(device, C.byref(self.ctx))
        if rc:
            raise BpGpuError(rc, _lib.bpgpu_strerror(rc).decode())

    @classmethod
    def borrowed(cls, ctx):
        """a BpGpu over a context that someone else owns (BpPool.ctx): close() leaves the context alone"""
        self = cls.__new__(cls)
        self.ctx, self._borrowed = C.c_void_p(ctx), True
        return self

    def close(self):
        if self.ctx:
            if not getattr(self, "_borrowed", False):
                _lib.bpgpu_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc:
            raise BpGpuError(rc, _lib.bpgpu_strerror(rc).decode() + " | " + _lib.bpgpu_last_error(self.ctx).decode())

    # ---- plumbing
    def set_option(self, name, value):
        """launch-route option of this context (OPT keys; include/bpgpu.h BPGPU_OPT_*), or "horner_group" (bpgpu_set_horner_group)"""
        if name == "horner_group":
            return self.set_horner_group(value)
        self._ck(_lib.bpgpu_set_option(self.ctx, OPT[name], int(value)))

    def get_option(self, name):
        if name == "horner_group":
            return self.get_horner_group()
        v = C.c_int64()
        self._ck(_lib.bpgpu_get_option(self.ctx, OPT[name], C.byref(v)))
        return v.value

    def set_horner_group(self, windows):
        """windows per group of the first Horner stage: 8, 16, 32; 0 = by mode (include/bpgpu.h)"""
        windows = int(windows)
        if not -(1 << 31) <= windows < (1 << 31):
            raise BpGpuError(E_ARG, "set_horner_group: not a C int")
        self._ck(_lib.bpgpu_set_horner_group(self.ctx, windows))

    def get_horner_group(self):
        v = C.c_int()
        self._ck(_lib.bpgpu_get_horner_group(self.ctx, C.byref(v)))
        return v.value

    def options(self, **kw):
        """context manager: set options, restore the previous values on exit"""
        gpu = self

        class _Scope:
            def __enter__(s):
                s.old = {k: gpu.get_option(k) for k in kw}
                for k, v in kw.items():
                    gpu.set_option(k, v)
                return gpu

            def __exit__(s, *exc):
                for k, v in s.old.items():
                    gpu.set_option(k, v)
                return False
        return _Scope()

    def sync(self):
        self._ck(_lib.bpgpu_sync(self.ctx))

    def stream(self):
        return _lib.bpgpu_stream(self.ctx)

    def malloc(self, nbytes):
        p = C.c_void_p()
        self._ck(_lib.bpgpu_malloc(self.ctx, nbytes, C.byref(p)))
        return p

    def free(self, p):
        self._ck(_lib.bpgpu_free(self.ctx, p))

    def upload(self, dptr, data):
        self._ck(_lib.bpgpu_upload(self.ctx, dptr, _buf(data), len(data)))

    def upload_async(self, dptr, host_ptr, nbytes):
        """enqueue a copy from (page-locked) host memory on the context's stream; host_ptr: integer address / c_void_p"""
        self._ck(_lib.bpgpu_upload_async(self.ctx, dptr, host_ptr, nbytes))

    def to_device(self, data):
        p = self.malloc(len(data))
        self.upload(p, data)
        return p

    def download(self, dptr, nbytes):
        o = _out(nbytes)
        self._ck(_lib.bpgpu_download(self.ctx, o, dptr, nbytes))
        return bytes(o)[:nbytes]

    def input_flag(self):
        v = C.c_int(0)
        self._ck(_lib.bpgpu_input_flag(self.ctx, C.byref(v)))
        return v.value

    def set_latency_mode(self, on=True):
        self._ck(_lib.bpgpu_set_latency_mode(self.ctx, 1 if on else 0))

    def profile_enable(self, on=True):
        self._ck(_lib.bpgpu_profile_enable(self.ctx, 1 if on else 0))

    def profile_select(self, names=None):
        """restrict the event timing to the named kinds (PROF_NAMES); None = all"""
        mask = 0xffffffff if names is None else sum(1 << PROF_NAMES.index(n) for n in names)
        self._ck(_lib.bpgpu_profile_select(self.ctx, mask))

    def profile_read(self):
        ms = (C.c_double * PROF_KINDS)()
        cnt = (C.c_uint64 * PROF_KINDS)()
        self._ck(_lib.bpgpu_profile_read(self.ctx, ms, cnt))
        return {n: (ms[i], int(cnt[i])) for i, n in enumerate(PROF_NAMES)}

    def profile_epoch(self):
        """reference event for profile_intervals (of any context of this device); owned by the context"""
        e = _lib.bpgpu_profile_epoch(self.ctx)
        if not e:
            raise BpGpuError(E_DEVICE, "bpgpu_profile_epoch")
        return C.c_void_p(e)

    def profile_intervals(self, epoch, cap=8192):
        """-> [(kind name, start ms, end ms)] of every timed launch since the last read, relative to `epoch`"""
        kind, a, b, n = (C.c_int32 * cap)(), (C.c_double * cap)(), (C.c_double * cap)(), C.c_size_t(0)
        self._ck(_lib.bpgpu_profile_intervals(self.ctx, epoch, cap, kind, a, b, C.byref(n)))
        return [(PROF_NAMES[kind[i]], a[i], b[i]) for i in range(n.value)]

    # ---- scalar field
    def batch_inverse(self, scalars):
        n = len(scalars) // 32
        b = _inout(scalars)
        self._ck(_lib.bpgpu_batch_inverse(self.ctx, b, n))
        return bytes(b)[:32 * n]

    def msm_batch_dev(self, nb, n, d_scalars, d_points, d_out):
        self._ck(_lib.bpgpu_msm_batch_dev(self.ctx, nb, n, d_scalars, d_points, d_out))

    # ---- arkworks in-memory forms (include/bpgpu.h): scalars 32 B = x 2^256 mod n, points 96 B = Jacobian coords c 2^256 mod p
    def msm_ark(self, scalars_mont, points_jac_mont):
        n = len(scalars_mont) // 32
        if len(points_jac_mont) != 96 * n:
            raise BpGpuError(E_LEN, "msm_ark: length mismatch")
        o = _out(96)
        self._ck(_lib.bpgpu_msm_ark(self.ctx, _buf(scalars_mont), _buf(points_jac_mont), n, o))
        return bytes(o)

    def _ark(self, fn, data, isz, osz):
        n = len(data) // isz
        o = _out(osz * n)
        self._ck(fn(self.ctx, _buf(data), n, o))
        return bytes(o)[:osz * n]

    def scalars_from_ark(self, b):
        return self._ark(_lib.bpgpu_scalars_from_ark, b, 32, 32)

    def scalars_to_ark(self, b):
        return self._ark(_lib.bpgpu_scalars_to_ark, b, 32, 32)

    def points_from_ark(self, b):
        return self._ark(_lib.bpgpu_points_from_ark, b, 96, 64)

    def points_to_ark(self, b):
        return self._ark(_lib.bpgpu_points_to_ark, b, 64, 96)

    def points_sum(self, points):
        """sum of the 64-byte points in `points` (no scalars) -> 64 bytes"""
        n = len(points) // 64
        out = _out(64)
        self._ck(_lib.bpgpu_points_sum(self.ctx, _buf(points), n, out))
        return bytes(out)

    def msm_shared(self, nsets, n, scalars, points):
        """nsets MSMs over one point vector (msm_authenticated_iter's share / MAC / modifier MSMs)."""
        out = _out(64 * nsets)
        self._ck(_lib.bpgpu_msm_shared(self.ctx, nsets, n, _buf(scalars), _buf(points), out))
        return bytes(out)[:64 * nsets]

    def points_decompress(self, compressed):
        """-> (xy bytes n x 64, ok list) for n x 32-byte compressed points"""
        n = len(compressed) // 32
        xy, ok = _out(64 * n), (C.c_int32 * max(n, 1))()
        self._ck(_lib.bpgpu_points_decompress(self.ctx, _buf(compressed), n, xy, ok))
        return bytes(xy)[:64 * n], list(ok)[:n]

    def points_compress(self, xy):
        n = len(xy) // 64
        out = _out(32 * n)
        self._ck(_lib.bpgpu_points_compress(self.ctx, _buf(xy), n, out))
        return bytes(out)[:32 * n]

    def inner_product(self, a, b):
        if len(a) != len(b):
            raise BpGpuError(E_LEN, "inner_product(a,b): lengths of vectors do not match")
        o = _out(32)
        self._ck(_lib.bpgpu_inner_product(self.ctx, _buf(a), _buf(b), len(a) // 32, o))
        return bytes(o)

    # ---- MSM
    def msm(self, scalars, points):
        n = len(scalars) // 32
        if len(points) != 64 * n:
            raise BpGpuError(E_LEN, "msm: length mismatch")
        o = _out(64)
        self._ck(_lib.bpgpu_msm(self.ctx, _buf(scalars), _buf(points), n, o))
        return bytes(o)

    def msm_batch(self, nb, n, scalars, points):
        if len(scalars) != 32 * nb * n or len(points) != 64 * nb * n:
            raise BpGpuError(E_LEN, "msm_batch: length mismatch")
        o = _out(64 * nb)
        self._ck(_lib.bpgpu_msm_batch(self.ctx, nb, n, _buf(scalars), _buf(points), o))
        return bytes(o)[:64 * nb]

    # ---- generators
    def gens_create(self, G, H, B, B_blinding, window_bits=8):
        cap = len(G) // 64
        h = C.c_void_p()
        self._ck(_lib.bpgpu_gens_create(self.ctx, _buf(G), _buf(H), cap, _buf(B), _buf(B_blinding), window_bits, C.byref(h)))
        return h

    def gens_destroy(self, h):
        _lib.bpgpu_gens_destroy(self.ctx, h)

    def msm_gens(self, gens, nb, n, scalars, ark=False):
        """ark=True: the scalars are ark-ff Montgomery limbs (x * 2^256 mod n), converted on the device"""
        o = _out(64 * nb)
        fn = _lib.bpgpu_msm_gens_ark if ark else _lib.bpgpu_msm_gens
        self._ck(fn(self.ctx, gens, nb, n, _buf(scalars), o))
        return bytes(o)[:64 * nb]

    # ---- IPP
    def fold_witness(self, n, u, u_inv, a, b, G, H):
        if not (len(a) == len(b) == 64 * n and len(G) == len(H) == 128 * n):
            raise BpGpuError(E_LEN, "fold_witness: length mismatch")
        ao, bo, Go, Ho = _out(32 * n), _out(32 * n), _out(64 * n), _out(64 * n)
        self._ck(_lib.bpgpu_fold_witness(self.ctx, n, _buf(u), _buf(u_inv), _buf(a), _buf(b), _buf(G), _buf(H), ao, bo, Go, Ho))
        return bytes(ao)[:32 * n], bytes(bo)[:32 * n], bytes(Go)[:64 * n], bytes(Ho)[:64 * n]

    def verification_scalars(self, challenges, n):
        k = len(challenges) // 32
        a, b, s = _out(32 * k), _out(32 * k), _out(32 * n)
        self._ck(_lib.bpgpu_verification_scalars(self.ctx, _buf(challenges), k, n, a, b, s))
        return bytes(a)[:32 * k], bytes(b)[:32 * k], bytes(s)[:32 * n]

    # lock-step InnerProductProof::create (transcript on the host)
    def ipp_begin(self, nb, n, Q, Gf, Hf, G, H, shared_gens, a, b):
        h = C.c_void_p()
        self._ck(_lib.bpgpu_ipp_begin(self.ctx, nb, n, _buf(Q), _buf(Gf), _buf(Hf), _buf(G), _buf(H), 1 if shared_gens else 0, _buf(a), _buf(b),
                                      C.byref(h)))
        return h

    def ipp_begin_gens(self, gens, nb, n, w, Gf, Hf, a, b):
        """Resident-generator session: G, H = gens[:n], Q = w * B (no generator folding on the device)."""
        h = C.c_void_p()
        self._ck(_lib.bpgpu_ipp_begin_gens(self.ctx, gens, nb, n, _buf(w), _buf(Gf), _buf(Hf), _buf(a), _buf(b), C.byref(h)))
        return h

    def ipp_len(self, s):
        return _lib.bpgpu_ipp_len(s)

    def ipp_round(self, s, nb):
        L, R = _out(64 * nb), _out(64 * nb)
        self._ck(_lib.bpgpu_ipp_round(self.ctx, s, L, R))
        return bytes(L)[:64 * nb], bytes(R)[:64 * nb]

    def ipp_fold(self, s, u, u_inv):
        self._ck(_lib.bpgpu_ipp_fold(self.ctx, s, _buf(u), _buf(u_inv)))

    def ipp_finish(self, s, nb):
        a, b = _out(32 * nb), _out(32 * nb)
        self._ck(_lib.bpgpu_ipp_finish(self.ctx, s, a, b))
        return bytes(a)[:32 * nb], bytes(b)[:32 * nb]

    def ipp_folded_gens(self, s, nb):
        G, H = _out(64 * nb), _out(64 * nb)
        self._ck(_lib.bpgpu_ipp_folded_gens(self.ctx, s, G, H))
        return bytes(G)[:64 * nb], bytes(H)[:64 * nb]

    def ipp_run_fs(self, s, nb, k, states):
        """all rounds with the transcript on the device -> (L bytes nb*k*64, R, a, b, states_out)"""
        L, R = _out(64 * nb * max(k, 1)), _out(64 * nb * max(k, 1))
        a, b, so = _out(32 * nb), _out(32 * nb), _out(32 * nb)
        self._ck(_lib.bpgpu_ipp_run_fs(self.ctx, s, _buf(states), L, R, a, b, so))
        return bytes(L)[:64 * nb * k], bytes(R)[:64 * nb * k], bytes(a)[:32 * nb], bytes(b)[:32 * nb], bytes(so)[:32 * nb]

    def ipp_destroy(self, s):
        _lib.bpgpu_ipp_destroy(self.ctx, s)

    # InnerProductProof::verify for nb proofs of one length n = 2^k (include/bpgpu.h bpgpu_ipp_verify_*)
    @staticmethod
    def _opt(b):
        return _buf(b) if b else None

    def ipp_verify_batch(self, nb, n, Q, Gf, Hf, G, H, shared_gens, P, L, R, ab, challenges, want_expect=False, k=None):
        """-> accept bits [nb] (and expect_P, nb x 64 B, with want_expect).  L, R, challenges: nb x k entries, proof-major."""
        k = n.bit_length() - 1 if k is None else k
        ok, ex = (C.c_int32 * max(nb, 1))(), _out(64 * nb) if want_expect else None
        self._ck(_lib.bpgpu_ipp_verify_batch(self.ctx, nb, n, k, _buf(Q), _buf(Gf), _buf(Hf), _buf(G), _buf(H), 1 if shared_gens else 0, _buf(P),
                                             self._opt(L), self._opt(R), _buf(ab), self._opt(challenges), ok, ex))
        return (list(ok)[:nb], bytes(ex)[:64 * nb]) if want_expect else list(ok)[:nb]

    def ipp_verify_batch_dev(self, nb, n, k, d_Q, d_Gf, d_Hf, d_G, d_H, shared_gens, d_P, d_L, d_R, d_ab, d_challenges, d_ok, d_expect=None):
        """device pointers, asynchronous: sync() before reading d_ok; malformed operands raise input_flag()"""
        self._ck(_lib.bpgpu_ipp_verify_batch_dev(self.ctx, nb, n, k, d_Q, d_Gf, d_Hf, d_G, d_H, 1 if shared_gens else 0, d_P, d_L, d_R, d_ab,
                                                 d_challenges, d_ok, d_expect))

    def ipp_verify_gens(self, gens, nb, n, w, Gf, Hf, P, L, R, ab, challenges, want_expect=False):
        """over resident generators: G, H = gens[:n], Q = w * B"""
        k = n.bit_length() - 1
        ok, ex = (C.c_int32 * max(nb, 1))(), _out(64 * nb) if want_expect else None
        self._ck(_lib.bpgpu_ipp_verify_gens(self.ctx, gens, nb, n, k, _buf(w), _buf(Gf), _buf(Hf), _buf(P), self._opt(L), self._opt(R), _buf(ab),
                                            self._opt(challenges), ok, ex))
        return (list(ok)[:nb], bytes(ex)[:64 * nb]) if want_expect else list(ok)[:nb]

    def ipp_verify_fs(self, gens, nb, n, Q_or_w, Gf, Hf, G, H, shared_gens, P, L, R, ab, states):
        """transcript replay on the device from `states` (after innerproduct_domain_sep) -> (accept bits, states_out);
        gens None: Q and G, H as ipp_verify_batch; else resident generators and w"""
        k = n.bit_length() - 1
        ok, so = (C.c_int32 * max(nb, 1))(), _out(32 * nb)
        self._ck(_lib.bpgpu_ipp_verify_fs(self.ctx, gens, nb, n, k, _buf(Q_or_w), _buf(Gf), _buf(Hf), self._opt(G), self._opt(H),
                                          1 if shared_gens else 0, _buf(P), self._opt(L), self._opt(R), _buf(ab), _buf(states), ok, so))
        return list(ok)[:nb], bytes(so)[:32 * nb]

    def generator_mul(self, scalars):
        n = len(scalars) // 32
        o = _out(64 * n)
        self._ck(_lib.bpgpu_generator_mul(self.ctx, _buf(scalars), n, o))
        return bytes(o)[:64 * n]

    def prover_polys(self, circuit, nb, n, m, y, y_inv, z, a_L, a_R, a_O, s_L, s_R):
        t, wV, h = _out(32 * 6 * nb), _out(32 * nb * m), C.c_void_p()
        self._ck(_lib.bpgpu_r1cs_prover_polys(self.ctx, circuit, nb, _buf(y), _buf(y_inv), _buf(z), _buf(a_L), _buf(a_R), _buf(a_O), _buf(s_L),
                                              _buf(s_R), t, wV, C.byref(h)))
        return bytes(t)[:32 * 6 * nb], bytes(wV)[:32 * nb * m], h

    def prover_eval(self, sess, nb, padded_n, x):
        lv, rv = _out(32 * nb * padded_n), _out(32 * nb * padded_n)
        self._ck(_lib.bpgpu_r1cs_prover_eval(self.ctx, sess, padded_n, _buf(x), lv, rv))
        return bytes(lv)[:32 * nb * padded_n], bytes(rv)[:32 * nb * padded_n]

    def prover_destroy(self, sess):
        _lib.bpgpu_prover_destroy(self.ctx, sess)

    # ---- R1CS
    def circuit_create(self, row_ptr, kind, idx, coeff, n_mul, m, ark=False):
        """ark=True: coefficients as ark-ff Montgomery limbs (x * 2^256 mod n)"""
        q = len(row_ptr) - 1
        nnz = len(kind)
        h = C.c_void_p()
        rp = (C.c_uint32 * (q + 1))(*row_ptr)
        kd = (C.c_uint32 * max(nnz, 1))(*kind)
        ix = (C.c_uint32 * max(nnz, 1))(*idx)
        fn = _lib.bpgpu_circuit_create_ark if ark else _lib.bpgpu_circuit_create
        self._ck(fn(self.ctx, q, rp, kd, ix, _buf(coeff), n_mul, m, C.byref(h)))
        return h

    def circuit_destroy(self, h):
        _lib.bpgpu_circuit_destroy(self.ctx, h)

    def flatten_constraints(self, circuit, n_mul, m, z, want_wc=True):
        nb = len(z) // 32
        wL, wR, wO = _out(32 * nb * n_mul), _out(32 * nb * n_mul), _out(32 * nb * n_mul)
        wV, wc = _out(32 * nb * m), _out(32 * nb)
        self._ck(_lib.bpgpu_flatten_constraints(self.ctx, circuit, nb, _buf(z), wL, wR, wO, wV, wc if want_wc else None))

        def cut(b, k):
            return bytes(b)[:32 * nb * k]

        return cut(wL, n_mul), cut(wR, n_mul), cut(wO, n_mul), cut(wV, m), bytes(wc)[:32 * nb]

    def r1cs_prover_polys(self, circuit, nb, n, m, y, y_inv, z, a_L, a_R, a_O, s_L, s_R, ark=False):
        """prover.rs:587-619 for nb provers of one circuit -> (t_coeffs nb x 6 x 32 B, wV nb x m x 32 B, prover handle);
        ark=True: every input scalar in ark-ff Montgomery form"""
        for v in (a_L, a_R, a_O, s_L, s_R):
            if len(v) != 32 * nb * n:
                raise BpGpuError(E_LEN, "r1cs_prover_polys: length mismatch")
        t, wv, h = _out(32 * 6 * nb), _out(32 * nb * max(m, 1)), C.c_void_p()
        fn = _lib.bpgpu_r1cs_prover_polys_ark if ark else _lib.bpgpu_r1cs_prover_polys
        self._ck(fn(self.ctx, circuit, nb, _buf(y), _buf(y_inv), _buf(z), _buf(a_L), _buf(a_R), _buf(a_O), _buf(s_L), _buf(s_R), t, wv, C.byref(h)))
        return bytes(t)[:32 * 6 * nb], bytes(wv)[:32 * nb * m], h

    def r1cs_prover_eval(self, prover, nb, padded_n, x):
        """prover.rs:659-672: l_vec, r_vec (nb x padded_n) = l(x), r(x) with the zero / -y^i padding"""
        lv, rv = _out(32 * nb * padded_n), _out(32 * nb * padded_n)
        self._ck(_lib.bpgpu_r1cs_prover_eval(self.ctx, prover, padded_n, _buf(x), lv, rv))
        return bytes(lv)[:32 * nb * padded_n], bytes(rv)[:32 * nb * padded_n]

    def r1cs_prover_commit(self, gens, session, nb, n_new, a_L, a_R, a_O, blindings, s_L=None, s_R=None, vector_keys=None):
        """prover.rs:457-494 / :519-565 on a resident-witness session (None: open one) -> (session, A_I A_O S nb x 3 x 64 B).
        All scalars in ark-ff Montgomery form; the blinding vectors explicit (s_L, s_R) or from vector_keys (nb x 32 B)."""
        h = session if session is not None else C.c_void_p()
        out = _out(64 * 3 * nb)
        opt = lambda b: _buf(b) if b is not None else None     # noqa: E731
        self._ck(_lib.bpgpu_r1cs_prover_commit(self.ctx, gens, C.byref(h), nb, n_new, opt(a_L), opt(a_R), opt(a_O), opt(s_L), opt(s_R),
                                               opt(vector_keys), _buf(blindings), out))
        return h, bytes(out)[:64 * 3 * nb]

    def r1cs_prover_ipp_begin(self, session, gens, padded_n, n1, x, u, y_inv, w):
        """prover.rs:659-708 on the device: l(x), r(x), G / H factors and the resident-generator IPP session (y_inv None: the session's)"""
        h = C.c_void_p()
        self._ck(_lib.bpgpu_r1cs_prover_ipp_begin(self.ctx, session, gens, padded_n, n1, _buf(x), _buf(u), _buf(y_inv) if y_inv is not None else None,
                                                  _buf(w), C.byref(h)))
        return h

    def r1cs_prover_session_polys(self, session, circuit, nb, m, y, z):
        """prover.rs:587-619 on the session's planes -> (t_coeffs nb x 6 x 32 B, wV nb x m x 32 B); y, z canonical LE"""
        t, wv = _out(32 * 6 * nb), _out(32 * nb * max(m, 1))
        self._ck(_lib.bpgpu_r1cs_prover_session_polys(self.ctx, session, circuit, _buf(y), _buf(z), t, wv))
        return bytes(t)[:32 * 6 * nb], bytes(wv)[:32 * nb * m]

    def r1cs_prover_session_polys_param(self, session, circuit, nb, m, y, z, gadget_challenges):
        """the same for a circuit of circuit_create_param; gadget_challenges nb x nchi x 32 B canonical LE"""
        t, wv = _out(32 * 6 * nb), _out(32 * nb * max(m, 1))
        self._ck(_lib.bpgpu_r1cs_prover_session_polys_param(self.ctx, session, circuit, _buf(y), _buf(z), _buf(gadget_challenges), t, wv))
        return bytes(t)[:32 * 6 * nb], bytes(wv)[:32 * nb * m]

    def r1cs_prove_fs(self, gens, circuit, nb, n, m, states, a_L, a_R, a_O, blindings, v_blinding=None, s_L=None, s_R=None,
                      vector_keys=None, want_wire=True):
        """Prover::prove in one call for nb provers of a one-phase circuit of n multipliers and m commitments, transcript on the
        device (include/bpgpu.h bpgpu_r1cs_prove_fs).  Witness, v_blinding and blindings (nb x 8) in ark-ff Montgomery form, the
        blinding vectors explicit or from vector_keys -> (proof_points nb x (11 + 2k) x 64 B, proof_scalars nb x 5 x 32 B, wire
        nb x proof_len or None, challenges nb x (5 + k) x 32 B, states_out nb x 32 B)"""
        k = max(n - 1, 0).bit_length()
        nvar, plen = 11 + 2 * k, 1 + 11 * 32 + (2 * k + 2) * 32
        pts, sc, ch, so = _out(64 * nb * nvar), _out(160 * nb), _out(32 * nb * (5 + k)), _out(32 * nb)
        wire = _out(nb * plen) if want_wire else None
        opt = lambda b: _buf(b) if b is not None else None     # noqa: E731
        self._ck(_lib.bpgpu_r1cs_prove_fs(self.ctx, gens, circuit, nb, opt(states), opt(a_L), opt(a_R), opt(a_O), opt(s_L), opt(s_R),
                                          opt(vector_keys), opt(v_blinding), opt(blindings), pts, sc, wire, ch, so))
        return (bytes(pts)[:64 * nb * nvar], bytes(sc)[:160 * nb], bytes(wire)[:nb * plen] if want_wire else None,
                bytes(ch)[:32 * nb * (5 + k)], bytes(so)[:32 * nb])

    def r1cs_prove_fs_dev(self, gens, circuit, nb, d_states, d_a_L, d_a_R, d_a_O, d_blindings, d_points, d_scalars, d_v_blinding=None,
                          d_s_L=None, d_s_R=None, d_vector_keys=None, d_wire=None, d_ch=None, d_states_out=None):
        """the same on device pointers, asynchronous on the context's stream; a malformed operand raises input_flag()"""
        self._ck(_lib.bpgpu_r1cs_prove_fs_dev(self.ctx, gens, circuit, nb, d_states, d_a_L, d_a_R, d_a_O, d_s_L, d_s_R, d_vector_keys, d_v_blinding,
                                              d_blindings, d_points, d_scalars, d_wire, d_ch, d_states_out))

    def r1cs_commit_values(self, gens, nb, m, v, v_blinding, states=None, want_points=True, want_compressed=True):
        """Prover::commit for the m values of each of nb provers (include/bpgpu.h bpgpu_r1cs_commit_values): v, v_blinding nb x m in
        ark-ff Montgomery form, states nb x 32 B the chain on entry to Prover::new (or None: no transcript) -> (V nb x m x 64 B,
        V_compressed nb x m x 32 B, states_out nb x 32 B: the states of r1cs_prove_fs), each None when not asked for"""
        V = _out(64 * nb * m) if want_points else None
        Vc = _out(32 * nb * m) if want_compressed else None
        so = _out(32 * nb) if states is not None else None
        opt = lambda b: _buf(b) if b is not None else None     # noqa: E731
        self._ck(_lib.bpgpu_r1cs_commit_values(self.ctx, gens, nb, m, opt(v), opt(v_blinding), opt(states), V, Vc, so))
        return (bytes(V)[:64 * nb * m] if want_points else None, bytes(Vc)[:32 * nb * m] if want_compressed else None,
                bytes(so)[:32 * nb] if states is not None else None)

    def r1cs_commit_values_dev(self, gens, nb, m, d_v, d_v_blinding, d_states=None, d_V=None, d_V_compressed=None, d_states_out=None):
        """the same on device pointers, asynchronous on the context's stream; a malformed operand raises input_flag()"""
        self._ck(_lib.bpgpu_r1cs_commit_values_dev(self.ctx, gens, nb, m, d_v, d_v_blinding, d_states, d_V, d_V_compressed, d_states_out))

    def r1cs_prove_fs2_begin(self, gens, circuit, nb, n1, states, gadget_label, blindings, a_L=None, a_R=None, a_O=None, s_L=None, s_R=None,
                             vector_keys=None, nchi=1):
        """The first of the two calls that prove nb provers of a two-phase circuit (include/bpgpu.h bpgpu_r1cs_prove_fs2_begin): the
        phase-1 commitments over n1 multipliers and the device transcript up to the gadget's challenge.  Witness and blindings
        (nb x 3) in ark-ff Montgomery form -> (session, A_I1 A_O1 S1 nb x 3 x 64 B, gadget challenges nb x nchi x 32 B, states nb x 32 B).
        gadget_label None: the nchi labels attached to the circuit (circuit_set_gadget_labels)"""
        h = C.c_void_p()
        com, chi, so = _out(64 * 3 * nb), _out(32 * nb * nchi), _out(32 * nb)
        opt = lambda b: _buf(b) if b is not None else None     # noqa: E731
        self._ck(_lib.bpgpu_r1cs_prove_fs2_begin(self.ctx, gens, circuit, nb, n1, opt(states), _label(gadget_label), opt(a_L), opt(a_R), opt(a_O), opt(s_L),
                                                 opt(s_R), opt(vector_keys), opt(blindings), C.byref(h), com, chi, so))
        return (h if h.value else None), bytes(com)[:64 * 3 * nb], bytes(chi)[:32 * nb * nchi], bytes(so)[:32 * nb]

    def r1cs_prove_fs2_begin_dev(self, gens, circuit, nb, n1, d_states, gadget_label, d_blindings, d_a_L=None, d_a_R=None, d_a_O=None,
                                 d_s_L=None, d_s_R=None, d_vector_keys=None, d_commitments=None, d_chi=None, d_states_out=None):
        """the same on device pointers, asynchronous on the context's stream -> session; a malformed operand raises input_flag()"""
        h = C.c_void_p()
        self._ck(_lib.bpgpu_r1cs_prove_fs2_begin_dev(self.ctx, gens, circuit, nb, n1, d_states, _label(gadget_label), d_a_L, d_a_R, d_a_O, d_s_L, d_s_R,
                                                     d_vector_keys, d_blindings, C.byref(h), d_commitments, d_chi, d_states_out))
        return h if h.value else None

    def r1cs_prove_fs2_finish(self, gens, circuit, session, nb, n, m, a_L, a_R, a_O, blindings, v_blinding=None, s_L=None, s_R=None,
                              vector_keys=None, want_wire=True):
        """The second call (bpgpu_r1cs_prove_fs2_finish): the phase-2 witness (nb x n2), blindings nb x 8, on a session of
        r1cs_prove_fs2_begin for a circuit of n multipliers and m commitments -> (proof_points nb x (11 + 2k) x 64 B, proof_scalars
        nb x 5 x 32 B, wire nb x proof_len or None, challenges nb x (5 + k) x 32 B, states_out nb x 32 B).  `session` (a c_void_p) is
        cleared once the call has launched anything; after a refusal it stays open."""
        k = max(n - 1, 0).bit_length()
        nvar, plen = 11 + 2 * k, 1 + 14 * 32 + (2 * k + 2) * 32
        pts, sc, ch, so = _out(64 * nb * nvar), _out(160 * nb), _out(32 * nb * (5 + k)), _out(32 * nb)
        wire = _out(nb * plen) if want_wire else None
        opt = lambda b: _buf(b) if b is not None else None     # noqa: E731
        self._ck(_lib.bpgpu_r1cs_prove_fs2_finish(self.ctx, gens, circuit, C.byref(session) if session is not None else None, opt(a_L), opt(a_R),
                                                  opt(a_O), opt(s_L), opt(s_R), opt(vector_keys), opt(v_blinding), opt(blindings), pts, sc,
                                                  wire, ch, so))
        return (bytes(pts)[:64 * nb * nvar], bytes(sc)[:160 * nb], bytes(wire)[:nb * plen] if want_wire else None,
                bytes(ch)[:32 * nb * (5 + k)], bytes(so)[:32 * nb])

    def r1cs_prove_fs2_finish_dev(self, gens, circuit, session, d_a_L, d_a_R, d_a_O, d_blindings, d_points, d_scalars, d_v_blinding=None,
                                  d_s_L=None, d_s_R=None, d_vector_keys=None, d_wire=None, d_ch=None, d_states_out=None):
        """the same on device pointers, asynchronous; may follow r1cs_prove_fs2_begin_dev without a sync()"""
        self._ck(_lib.bpgpu_r1cs_prove_fs2_finish_dev(self.ctx, gens, circuit, C.byref(session) if session is not None else None, d_a_L, d_a_R,
                                                      d_a_O, d_s_L, d_s_R, d_vector_keys, d_v_blinding, d_blindings, d_points, d_scalars,
                                                      d_wire, d_ch, d_states_out))

    def r1cs_constraints_satisfied(self, circuit, nb, q, a_L, a_R, a_O, v=None, gadget_challenges=None, want_residuals=False):
        """Prover::constraints_satisfied for nb provers of a circuit of q constraints (include/bpgpu.h
        bpgpu_r1cs_constraints_satisfied): witness planes nb x n and the committed values nb x m in ark-ff Montgomery form, gadget
        challenges nb x nchi x 32 B canonical LE for a parametric circuit -> (ok, first_bad_row, first_bad_gate as lists of nb
        integers, -1 = none; residuals nb x q x 32 B canonical LE or None)"""
        ok, row, gate = (C.c_int32 * max(nb, 1))(), (C.c_int64 * max(nb, 1))(), (C.c_int64 * max(nb, 1))()
        res = _out(32 * nb * q) if want_residuals else None
        opt = lambda b: _buf(b) if b is not None else None     # noqa: E731
        self._ck(_lib.bpgpu_r1cs_constraints_satisfied(self.ctx, circuit, nb, opt(a_L), opt(a_R), opt(a_O), opt(v), opt(gadget_challenges), ok,
                                                       row, gate, res))
        return list(ok)[:nb], list(row)[:nb], list(gate)[:nb], bytes(res)[:32 * nb * q] if want_residuals else None

    def r1cs_constraints_satisfied_dev(self, circuit, nb, d_a_L, d_a_R, d_a_O, d_ok, d_v=None, d_gadget_challenges=None, d_first_bad_row=None,
                                       d_first_bad_gate=None, d_residuals=None):
        """the same on device pointers (ok nb x int32, the indices nb x int64), asynchronous on the context's stream; a malformed
        operand raises input_flag()"""
        self._ck(_lib.bpgpu_r1cs_constraints_satisfied_dev(self.ctx, circuit, nb, d_a_L, d_a_R, d_a_O, d_v, d_gadget_challenges, d_ok,
                                                           d_first_bad_row, d_first_bad_gate, d_residuals))

    # ---- witness synthesis (include/bpgpu.h bpgpu_witness)
    def witness_create(self, n, n1, m, nchi, op, arg, row_ptr, kind, idx, coeff):
        """a resident gate program: n multipliers (the first n1 in phase 1) over m committed values; op, arg per gate; the rows
        2 i (left), 2 i + 1 (right) as a CSR of (1 + nchi) * 2 n rows, coefficients canonical LE"""
        h = C.c_void_p()
        self._ck(_lib.bpgpu_witness_create(self.ctx, n, n1, m, nchi, _buf(bytes(op)), _u32s(arg), _u32s(row_ptr), _u32s(kind), _u32s(idx),
                                           _buf(coeff), C.byref(h)))
        return h

    def witness_destroy(self, w):
        _lib.bpgpu_witness_destroy(self.ctx, w)

    def r1cs_witness_synthesize(self, w, nb, n, phase=0, v=None, inputs=None, gadget_challenges=None, a_L=None, a_R=None, a_O=None):
        """the witnesses of nb provers of a program of n multipliers (bpgpu_r1cs_witness_synthesize): v nb x m and inputs
        nb x n_inputs x 2 in ark form, gadget challenges nb x nchi x 32 B canonical LE -> (a_L, a_R, a_O) nb x n, ark form.  phase 1
        or 2 assigns that phase's gates only: the planes given (phase 2: holding phase 1) come back with the rest untouched"""
        planes = [_inout(p) if p is not None else _out(32 * nb * n) for p in (a_L, a_R, a_O)]
        opt = lambda b: _buf(b) if b is not None else None     # noqa: E731
        self._ck(_lib.bpgpu_r1cs_witness_synthesize(self.ctx, w, nb, phase, opt(v), opt(inputs), opt(gadget_challenges), *planes))
        return tuple(bytes(p)[:32 * nb * n] for p in planes)

    def r1cs_witness_synthesize_dev(self, w, nb, phase, d_a_L, d_a_R, d_a_O, d_v=None, d_inputs=None, d_gadget_challenges=None):
        """the same on device pointers, asynchronous on the context's stream; a malformed operand raises input_flag()"""
        self._ck(_lib.bpgpu_r1cs_witness_synthesize_dev(self.ctx, w, nb, phase, d_v, d_inputs, d_gadget_challenges, d_a_L, d_a_R, d_a_O))

    def r1cs_prove_fs2(self, gens, circuit, w, nb, n, m, states, gadget_label, blindings, v=None, inputs=None, v_blinding=None, s_L=None,
                       s_R=None, vector_keys=None, want_wire=True, want_witness=False, nchi=1):
        """Prover::prove for nb provers of a two-phase circuit of n multipliers and m commitments in one call (bpgpu_r1cs_prove_fs2):
        the gates of program w on the device around the two transcript chains; blindings nb x 11 -> (proof_points, proof_scalars, wire
        or None, challenges, states_out, gadget challenges nb x nchi x 32 B, (a_L, a_R, a_O) or None).  gadget_label None: the nchi
        labels attached to the circuit (circuit_set_gadget_labels)"""
        k = max(n - 1, 0).bit_length()
        nvar, plen = 11 + 2 * k, 1 + 14 * 32 + (2 * k + 2) * 32
        pts, sc, ch, so, chi = _out(64 * nb * nvar), _out(160 * nb), _out(32 * nb * (5 + k)), _out(32 * nb), _out(32 * nb * nchi)
        wire = _out(nb * plen) if want_wire else None
        planes = [_out(32 * nb * n) if want_witness else None for _ in range(3)]
        opt = lambda b: _buf(b) if b is not None else None     # noqa: E731
        self._ck(_lib.bpgpu_r1cs_prove_fs2(self.ctx, gens, circuit, w, nb, opt(states), _label(gadget_label), opt(v), opt(inputs), opt(s_L), opt(s_R),
                                           opt(vector_keys), opt(v_blinding), opt(blindings), pts, sc, wire, ch, so, chi, *planes))
        return (bytes(pts)[:64 * nb * nvar], bytes(sc)[:160 * nb], bytes(wire)[:nb * plen] if want_wire else None,
                bytes(ch)[:32 * nb * (5 + k)], bytes(so)[:32 * nb], bytes(chi)[:32 * nb * nchi],
                tuple(bytes(p)[:32 * nb * n] for p in planes) if want_witness else None)

    def r1cs_prove_fs2_dev(self, gens, circuit, w, nb, d_states, gadget_label, d_blindings, d_points, d_scalars, d_v=None, d_inputs=None,
                           d_v_blinding=None, d_s_L=None, d_s_R=None, d_vector_keys=None, d_wire=None, d_ch=None, d_states_out=None,
                           d_chi=None, d_a_L=None, d_a_R=None, d_a_O=None):
        """the same on device pointers, asynchronous on the context's stream; a malformed operand raises input_flag()"""
        self._ck(_lib.bpgpu_r1cs_prove_fs2_dev(self.ctx, gens, circuit, w, nb, d_states, _label(gadget_label), d_v, d_inputs, d_s_L, d_s_R, d_vector_keys,
                                               d_v_blinding, d_blindings, d_points, d_scalars, d_wire, d_ch, d_states_out, d_chi, d_a_L,
                                               d_a_R, d_a_O))

    def r1cs_prove_values(self, gens, circuit, w, nb, n, m, *, init_states, blindings, v=None, v_blinding=None, inputs=None,
                          gadget_label=None, s_L=None, s_R=None, vector_keys=None, want_wire=True, want_witness=False, dev=False,
                          d_out=None, nchi=None):
        """Commitments, verdicts and proofs of nb provers from their committed values in one call (bpgpu_r1cs_prove_values): the stages
        commit_values -> witness synthesis -> constraints_satisfied -> prove_fs (gadget_label None: a numeric circuit, blindings
        nb x 8), or commit_values -> the prove_fs2 chain -> constraints_satisfied (a label: a two-phase circuit, blindings nb x 11),
        resident in between -> ProveValues; the proof rows of a prover with ok == 0 are zero bytes.  Operands are bytes, or c_void_p
        of page-locked memory.  dev=True: every operand a bpgpu_malloc pointer and d_out a dict of device pointers under ProveValues'
        field names (a_L, a_R, a_O for the planes; ok, points and scalars required): asynchronous, nothing is returned.  nchi (with
        gadget_label None): a two-phase circuit with that many attached labels (circuit_set_gadget_labels), blindings nb x 11"""
        lab = _label(gadget_label)
        if dev:
            o = lambda name: d_out.get(name)     # noqa: E731
            self._ck(_lib.bpgpu_r1cs_prove_values_dev(self.ctx, gens, circuit, w, nb, init_states, lab, v, v_blinding, inputs, s_L, s_R,
                                                      vector_keys, blindings, o("V"), o("V_compressed"), o("ok"), o("first_bad_row"),
                                                      o("first_bad_gate"), o("points"), o("scalars"), o("wire"), o("challenges"), o("states"),
                                                      o("chi"), o("a_L"), o("a_R"), o("a_O")))
            return None
        return _prove_values_host(lambda *a: self._ck(_lib.bpgpu_r1cs_prove_values(self.ctx, gens, circuit, w, *a)), nb, n, m, lab, init_states,
                                  v, v_blinding, inputs, s_L, s_R, vector_keys, blindings, want_wire, want_witness, nchi)

    def prover_destroy(self, prover):
        _lib.bpgpu_prover_destroy(self.ctx, prover)

    # ---- two-party prover, one party's local work (include/bpgpu.h: three planes share | MAC | modifier per scalar, every share in
    # ark-ff Montgomery form, challenges canonical LE once per proof)
    def mpc_prover_commit(self, gens, session, nb, n_new, a_L, a_R, a_O, s_L, s_R, blindings):
        """mpc_prover.rs:621-657 / :717-750 -> (session, A_I A_O S as nb x 3 planes x 3 x 64 B); operands nb x 3 x n_new, blindings nb x 3 x 3"""
        h = session if session is not None else C.c_void_p()
        out = _out(64 * 9 * nb)
        opt = lambda b: _buf(b) if b is not None else None     # noqa: E731
        self._ck(_lib.bpgpu_mpc_prover_commit(self.ctx, gens, C.byref(h), nb, n_new, opt(a_L), opt(a_R), opt(a_O), opt(s_L), opt(s_R),
                                              _buf(blindings), out))
        return h, bytes(out)[:64 * 9 * nb]

    def mpc_constraints_eval(self, circuit, nb, q, a_L, a_R, a_O, v=None, gadget_challenges=None):
        """one party's local half of MpcProver::constraints_satisfied (mpc_prover.rs:556-568): operand planes nb x 3 x n, v nb x 3 x m
        -> the rows' values on the party's planes, nb x 3 x q, for the host to open and compare with zero"""
        res = _out(32 * nb * 3 * q)
        opt = lambda b: _buf(b) if b is not None else None     # noqa: E731
        self._ck(_lib.bpgpu_mpc_constraints_eval(self.ctx, circuit, nb, opt(a_L), opt(a_R), opt(a_O), opt(v), opt(gadget_challenges), res))
        return bytes(res)[:32 * nb * 3 * q]

    def mpc_commit_values(self, gens, nb, m, v, v_blinding):
        """one party's local half of MpcProver::batch_commit_preshared (mpc_prover.rs:402-456): v, v_blinding nb x 3 x m -> the
        commitments on the party's planes, nb x 3 x m x 64 B, for the host to open"""
        V = _out(64 * nb * 3 * m)
        opt = lambda b: _buf(b) if b is not None else None     # noqa: E731
        self._ck(_lib.bpgpu_mpc_commit_values(self.ctx, gens, nb, m, opt(v), opt(v_blinding), V))
        return bytes(V)[:64 * nb * 3 * m]

    # ---- two-party witness synthesis, a dependency level of a gate program per mask / combine pair (bpgpu_mpc_witness_*)
    def mpc_witness_begin(self, w, nb, phase=0, v=None, inputs=None, gadget_challenges=None, a_L=None, a_R=None, a_O=None):
        """a session over program w for nb proofs: v nb x 3 x m, inputs nb x 3 x n_inputs x 2, for phase 2 the planes nb x 3 x n
        holding phase 1 -> the session, or None when nb == 0"""
        h = C.c_void_p()
        opt = lambda b: _buf(b) if b is not None else None     # noqa: E731
        self._ck(_lib.bpgpu_mpc_witness_begin(self.ctx, w, nb, phase, opt(v), opt(inputs), opt(gadget_challenges), opt(a_L), opt(a_R),
                                              opt(a_O), C.byref(h)))
        return h if h.value else None

    def mpc_witness_levels_left(self, s):
        return _lib.bpgpu_mpc_witness_levels_left(s)

    def mpc_witness_level_len(self, s):
        """the gates G of the level the next mpc_witness_mask evaluates; 0 when none is left"""
        return _lib.bpgpu_mpc_witness_level_len(s)

    def mpc_witness_mask(self, s, nb, triples):
        """triples nb x 3 (x, y, z) x 3 x G -> masked nb x 2 (d, e) x 3 x G"""
        g = self.mpc_witness_level_len(s)
        out = _out(32 * nb * 6 * g)
        self._ck(_lib.bpgpu_mpc_witness_mask(self.ctx, s, _buf(triples), out))
        return bytes(out)[:32 * nb * 6 * g]

    def mpc_witness_combine(self, s, opened):
        """opened nb x 2 (d, e) x G: a_O of the level's gates; the session advances to the next level"""
        self._ck(_lib.bpgpu_mpc_witness_combine(self.ctx, s, _buf(opened)))

    def mpc_witness_finish(self, s, nb, n):
        """-> (a_L, a_R, a_O) nb x 3 x n"""
        planes = [_out(32 * nb * 3 * n) for _ in range(3)]
        self._ck(_lib.bpgpu_mpc_witness_finish(self.ctx, s, *planes))
        return tuple(bytes(p)[:32 * nb * 3 * n] for p in planes)

    def mpc_witness_destroy(self, s):
        _lib.bpgpu_mpc_witness_destroy(self.ctx, s)

    def mpc_prover_polys_mask(self, session, circuit, nb, n, y, z, triples, gadget_challenges=None):
        """mpc_prover.rs:783-829: triples nb x 6 x 3 x 3 x n -> masked d, e (nb x 6 x 2 x 3 x n)"""
        out = _out(32 * nb * 36 * max(n, 1))
        self._ck(_lib.bpgpu_mpc_prover_polys_mask(self.ctx, session, circuit, _buf(y), _buf(z),
                                                  _buf(gadget_challenges) if gadget_challenges is not None else None, _buf(triples), out))
        return bytes(out)[:32 * nb * 36 * n]

    def mpc_prover_polys_finish(self, session, nb, m, opened, t_blindings):
        """opened d, e (nb x 6 x 2 x n), t_blindings (nb x 3 x 5) -> (t_coeffs nb x 3 x 6, T nb x 3 x 5 x 64 B, wV nb x m canonical)"""
        t, T, wv = _out(32 * 18 * nb), _out(64 * 15 * nb), _out(32 * nb * max(m, 1))
        self._ck(_lib.bpgpu_mpc_prover_polys_finish(self.ctx, session, _buf(opened), _buf(t_blindings), t, T, wv))
        return bytes(t)[:32 * 18 * nb], bytes(T)[:64 * 15 * nb], bytes(wv)[:32 * nb * m]

    def mpc_prover_ipp_begin(self, session, gens, padded_n, n1, x, u, w):
        """mpc_prover.rs:901-917 + the SharedInnerProductProof set-up -> IPP session of 3 planes per proof"""
        h = C.c_void_p()
        self._ck(_lib.bpgpu_mpc_prover_ipp_begin(self.ctx, session, gens, padded_n, n1, _buf(x), _buf(u), _buf(w), C.byref(h)))
        return h

    def mpc_ipp_mask(self, s, nb, triples):
        """triples nb x 2 x 3 x 3 x h -> masked nb x 2 x 2 x 3 x h (c_L, c_R)"""
        h = self.ipp_len(s) // 2
        out = _out(32 * nb * 12 * max(h, 1))
        self._ck(_lib.bpgpu_mpc_ipp_mask(self.ctx, s, _buf(triples), out))
        return bytes(out)[:32 * nb * 12 * h]

    def mpc_ipp_round(self, s, nb, opened):
        """opened nb x 2 x 2 x h -> (L, R) nb x 3 planes x 64 B each"""
        L, R = _out(64 * 3 * nb), _out(64 * 3 * nb)
        self._ck(_lib.bpgpu_mpc_ipp_round(self.ctx, s, _buf(opened), L, R))
        return bytes(L)[:192 * nb], bytes(R)[:192 * nb]

    def r1cs_verify_batch(self, gens, circuit, nb, n1, k, m, points, scalars, challenges, want_mega=True,
                          want_scalars=False):
        np_ = 1 << k
        nvar, nterms = 11 + m + 2 * k, 13 + m + 2 * np_ + 2 * k
        if len(points) != 64 * nb * nvar or len(scalars) != 160 * nb or len(challenges) != 32 * nb * (6 + k):
            raise BpGpuError(E_LEN, "r1cs_verify_batch: length mismatch")
        ok = (C.c_int32 * max(nb, 1))()
        mega = _out(64 * nb) if want_mega else None
        full = _out(32 * nb * nterms) if want_scalars else None
        self._ck(_lib.bpgpu_r1cs_verify_batch(self.ctx, gens, circuit, nb, n1, k, _buf(points), _buf(scalars), _buf(challenges), ok, mega, full))
        return (list(ok)[:nb], bytes(mega)[:64 * nb] if want_mega else None,
                bytes(full)[:32 * nb * nterms] if want_scalars else None)

    def r1cs_verify_batch_fs(self, gens, circuit, nb, n1, k, m, init_states, points, scalars, want_mega=True):
        nvar = 11 + m + 2 * k
        if len(points) != 64 * nb * nvar or len(scalars) != 160 * nb or len(init_states) != 32 * nb:
            raise BpGpuError(E_LEN, "r1cs_verify_batch_fs: length mismatch")
        ok = (C.c_int32 * max(nb, 1))()
        mega = _out(64 * nb) if want_mega else None
        ch = _out(32 * nb * (6 + k))
        self._ck(_lib.bpgpu_r1cs_verify_batch_fs(self.ctx, gens, circuit, nb, n1, k, _buf(init_states), _buf(points), _buf(scalars), ok, mega, ch))
        return list(ok)[:nb], (bytes(mega)[:64 * nb] if want_mega else None), bytes(ch)[:32 * nb * (6 + k)]

    def circuit_create_param(self, q, nchi, row_ptr, kind, idx, coeff, n_mul, m):
        """two-phase circuit with coefficients affine in nchi gadget challenges: a CSR of (1 + nchi) * q rows (include/bpgpu.h)"""
        nnz = len(kind)
        rp = (C.c_uint32 * len(row_ptr))(*row_ptr)
        kd = (C.c_uint32 * max(nnz, 1))(*kind)
        ix = (C.c_uint32 * max(nnz, 1))(*idx)
        h = C.c_void_p()
        self._ck(_lib.bpgpu_circuit_create_param(self.ctx, q, nchi, rp, kd, ix, _buf(coeff), n_mul, m, C.byref(h)))
        return h

    def circuit_set_gadget_labels(self, circuit, labels):
        """attach the labels of a parametric circuit's nchi gadget challenges, in draw order (bpgpu_circuit_set_gadget_labels): a list
        of byte strings, each zero-padded to 32 bytes; the device-transcript calls then take the circuit with gadget_label None"""
        tab = None if labels is None else _buf(b"".join((bytes(x) + bytes(32))[:32] for x in labels))
        self._ck(_lib.bpgpu_circuit_set_gadget_labels(self.ctx, circuit, tab))

    def r1cs_verify_batch_param(self, gens, circuit, nb, n1, k, m, points, scalars, challenges, gadget_challenges, want_mega=True,
                                want_scalars=False):
        np_ = 1 << k
        nterms = 13 + m + 2 * np_ + 2 * k
        ok = (C.c_int32 * max(nb, 1))()
        mega = _out(64 * nb) if want_mega else None
        full = _out(32 * nb * nterms) if want_scalars else None
        self._ck(_lib.bpgpu_r1cs_verify_batch_param(self.ctx, gens, circuit, nb, n1, k, _buf(points), _buf(scalars), _buf(challenges),
                                                    _buf(gadget_challenges), ok, mega, full))
        return (list(ok)[:nb], bytes(mega)[:64 * nb] if want_mega else None, bytes(full)[:32 * nb * nterms] if want_scalars else None)

    def r1cs_verify_batch_fs2(self, gens, circuit, nb, n1, k, m, nchi, init_states, gadget_label, points, scalars, want_mega=True):
        """-> (ok, mega, challenges nb x (6 + k) x 32, gadget challenges nb x nchi x 32)"""
        ok = (C.c_int32 * max(nb, 1))()
        mega = _out(64 * nb) if want_mega else None
        ch, chi = _out(32 * nb * (6 + k)), _out(32 * nb * max(nchi, 1))
        self._ck(_lib.bpgpu_r1cs_verify_batch_fs2(self.ctx, gens, circuit, nb, n1, k, _buf(init_states), _label(gadget_label), _buf(points), _buf(scalars), ok,
                                                  mega, ch, chi))
        return list(ok)[:nb], (bytes(mega)[:64 * nb] if want_mega else None), bytes(ch)[:32 * nb * (6 + k)], bytes(chi)[:32 * nb * nchi]

    def r1cs_verify_batch_fs_dev(self, gens, circuit, nb, n1, k, d_init, d_points, d_scalars, d_ok, d_mega=None, d_ch=None):
        self._ck(_lib.bpgpu_r1cs_verify_batch_fs_dev(self.ctx, gens, circuit, nb, n1, k, d_init, d_points, d_scalars, d_ok, d_mega, d_ch))

    def r1cs_verify_batch_wire(self, gens, circuit, nb, n1, proof_len, proofs, commitments, init_states):
        """wire-format proofs (R1CSProof::to_bytes) + compressed commitments -> accept bits, all on the device"""
        if len(proofs) != nb * proof_len or len(init_states) != 32 * nb:
            raise BpGpuError(E_LEN, "r1cs_verify_batch_wire: length mismatch")
        ok = (C.c_int32 * max(nb, 1))()
        self._ck(_lib.bpgpu_r1cs_verify_batch_wire(self.ctx, gens, circuit, nb, n1, proof_len, _buf(proofs), _buf(commitments), _buf(init_states),
                                                   ok))
        return list(ok)[:nb]

    def r1cs_verify_batch_wire_dev(self, gens, circuit, nb, n1, proof_len, d_proofs, d_commitments, d_init, d_ok):
        self._ck(_lib.bpgpu_r1cs_verify_batch_wire_dev(self.ctx, gens, circuit, nb, n1, proof_len, d_proofs, d_commitments, d_init, d_ok))

    def r1cs_verify_batch_wire2(self, gens, circuit, nb, n1, proof_len, gadget_label, proofs, commitments, init_states):
        """the same for a two-phase circuit (circuit_create_param): one gadget challenge drawn under gadget_label, or, with
        gadget_label None, the circuit's own under its attached labels (circuit_set_gadget_labels)"""
        if len(proofs) != nb * proof_len or len(init_states) != 32 * nb:
            raise BpGpuError(E_LEN, "r1cs_verify_batch_wire2: length mismatch")
        ok = (C.c_int32 * max(nb, 1))()
        self._ck(_lib.bpgpu_r1cs_verify_batch_wire2(self.ctx, gens, circuit, nb, n1, proof_len, _label(gadget_label), _buf(proofs), _buf(commitments),
                                                    _buf(init_states), ok))
        return list(ok)[:nb]

    def r1cs_verify_batch_wire2_dev(self, gens, circuit, nb, n1, proof_len, gadget_label, d_proofs, d_commitments, d_init, d_ok):
        self._ck(_lib.bpgpu_r1cs_verify_batch_wire2_dev(self.ctx, gens, circuit, nb, n1, proof_len, _label(gadget_label), d_proofs, d_commitments, d_init,
                                                        d_ok))

    def r1cs_verify_combined(self, gens, circuit, nb, n1, k, m, points, scalars, challenges, rho):
        nvar = 11 + m + 2 * k
        if len(points) != 64 * nb * nvar or len(scalars) != 160 * nb or len(challenges) != 32 * nb * (6 + k) or len(rho) != 32 * nb:
            raise BpGpuError(E_LEN, "r1cs_verify_combined: length mismatch")
        o = _out(64)
        self._ck(_lib.bpgpu_r1cs_verify_combined(self.ctx, gens, circuit, nb, n1, k, _buf(points), _buf(scalars), _buf(challenges), _buf(rho), o))
        return bytes(o)

    def r1cs_verify_combined_dev(self, gens, circuit, nb, n1, k, d_points, d_scalars, d_challenges, d_rho, d_out):
        self._ck(_lib.bpgpu_r1cs_verify_combined_dev(self.ctx, gens, circuit, nb, n1, k, d_points, d_scalars, d_challenges, d_rho, d_out))

    # ---- mixed queues: groups of proofs of several circuits in one call.  A group is a dict; the host forms take bytes, the _dev
    # forms device pointers (and ok: the group's nb int32 verdicts in HBM for the screened call).  Decoded operands: keys circuit, nb,
    # n1, k, points, scalars, challenges, rho and, for a parametric circuit, gadget_challenges (the layouts of r1cs_verify_batch).
    # Wire-format proofs: keys circuit, nb, n1, proof_len, proofs, commitments (None when m == 0), init_states, rho and, for a
    # parametric circuit, gadget_label (bytes, host memory in both forms).
    # A queue kind: (ctypes struct, its three size fields, its pointer fields, its host label or None)
    _DECODED = (VerifyGroup, ("nb", "n1", "k"), ("points", "scalars", "challenges", "gadget_challenges", "rho"), None)
    _WIRE = (WireGroup, ("nb", "n1", "proof_len"), ("proofs", "commitments", "init_states", "rho"), "gadget_label")

    @staticmethod
    def _queue(kind, groups, dev):
        struct, sizes, pointers, label = kind
        arr = (struct * max(len(groups), 1))()
        keep, oks = [], []
        for i, gr in enumerate(groups):
            g = arr[i]
            g.circuit = gr["circuit"]
            for f in sizes:
                setattr(g, f, gr[f])
            for f in pointers:
                v = gr.get(f)
                if v is None:
                    setattr(g, f, None)
                elif dev:
                    setattr(g, f, v)
                else:
                    b = C.create_string_buffer(bytes(v), max(len(v), 1))
                    keep.append(b)
                    setattr(g, f, C.cast(b, C.c_void_p).value)
            lab = gr.get(label) if label else None
            if lab is not None:
                b = C.create_string_buffer((bytes(lab) + bytes(32))[:32], 32)
                keep.append(b)
                setattr(g, label, C.cast(b, C.c_void_p).value)
            if dev:
                g.ok = gr.get("ok")
            else:
                ok = (C.c_int32 * max(gr["nb"], 1))()
                oks.append(ok)
                g.ok = C.cast(ok, C.c_void_p).value
        return arr, keep, oks

    def _queue_combined(self, fn, kind, gens, groups, d_out=None, dev=False):
        arr, keep, _ = self._queue(kind, groups, dev)
        o = d_out if dev else _out(64)
        self._ck(fn(self.ctx, gens, arr, len(groups), o))
        return None if dev else bytes(o)[:64]

    def _queue_screened(self, fn, kind, gens, groups, dev=False):
        arr, keep, oks = self._queue(kind, groups, dev)
        nf = C.c_size_t(0)
        self._ck(fn(self.ctx, gens, arr, len(groups), C.byref(nf)))
        return nf.value if dev else ([list(ok)[:gr["nb"]] for ok, gr in zip(oks, groups)], nf.value)

    def r1cs_verify_mixed_combined(self, gens, groups):
        """sum over all groups and proofs of rho_p * mega_check_p (64 bytes; all zero: every proof valid; 0xFF x 64: malformed input)"""
        return self._queue_combined(_lib.bpgpu_r1cs_verify_mixed_combined, self._DECODED, gens, groups)

    def r1cs_verify_mixed_combined_dev(self, gens, groups, d_out):
        self._queue_combined(_lib.bpgpu_r1cs_verify_mixed_combined_dev, self._DECODED, gens, groups, d_out, True)

    def r1cs_verify_mixed_screened(self, gens, groups):
        """-> ([ok list per group], number of checks that took the per-proof path)"""
        return self._queue_screened(_lib.bpgpu_r1cs_verify_mixed_screened, self._DECODED, gens, groups)

    def r1cs_verify_mixed_screened_dev(self, gens, groups):
        """verdicts into each group's device ok array (sync() before reading them) -> fallback checks"""
        return self._queue_screened(_lib.bpgpu_r1cs_verify_mixed_screened_dev, self._DECODED, gens, groups, True)

    def r1cs_verify_mixed_wire_combined(self, gens, groups):
        """sum over all groups and proofs of rho_p * mega_check_p from wire bytes (64 bytes; all zero: every proof valid; 0xFF x 64:
        an undecodable proof, an identity at a validated point or a malformed weight)"""
        return self._queue_combined(_lib.bpgpu_r1cs_verify_mixed_wire_combined, self._WIRE, gens, groups)

    def r1cs_verify_mixed_wire_combined_dev(self, gens, groups, d_out):
        self._queue_combined(_lib.bpgpu_r1cs_verify_mixed_wire_combined_dev, self._WIRE, gens, groups, d_out, True)

    def r1cs_verify_mixed_wire_screened(self, gens, groups):
        """-> ([ok list per group], number of checks that took the per-proof path)"""
        return self._queue_screened(_lib.bpgpu_r1cs_verify_mixed_wire_screened, self._WIRE, gens, groups)

    def r1cs_verify_mixed_wire_screened_dev(self, gens, groups):
        """verdicts into each group's device ok array (sync() before reading them) -> fallback checks"""
        return self._queue_screened(_lib.bpgpu_r1cs_verify_mixed_wire_screened_dev, self._WIRE, gens, groups, True)

    def set_shard(self, rank, world):
        """this context's share of ONE large proof split over the GPUs of a node (include/bpgpu.h bpgpu_set_shard)"""
        self._ck(_lib.bpgpu_set_shard(self.ctx, rank, world))

    def r1cs_verify_shard(self, gens, circuit, n1, k, points, scalars, challenges, rank, world, gadget_challenges=None):
        """rank's partial mega_check point of one proof (64 bytes)"""
        out = _out(64)
        self._ck(_lib.bpgpu_r1cs_verify_shard(self.ctx, gens, circuit, n1, k, _buf(points), _buf(scalars), _buf(challenges),
                                              _buf(gadget_challenges) if gadget_challenges is not None else None, rank, world, out))
        return bytes(out)[:64]

    def r1cs_verify_stream_dev(self, gens, circuit, nb, n1, k, d_points, d_scalars, d_challenges, d_ok):
        """any number of proofs in one call: batches over the context's ring of lanes (asynchronous; sync() waits for all)"""
        self._ck(_lib.bpgpu_r1cs_verify_stream_dev(self.ctx, gens, circuit, nb, n1, k, d_points, d_scalars, d_challenges, d_ok))

    def r1cs_verify_stream(self, gens, circuit, nb, n1, k, m, points, scalars, challenges, raw=False):
        """the same from host memory (bytes, or c_void_p of page-locked memory for all three operands) -> [ok]
        (raw = True: the nb x int32 verdicts as bytes -- turning 65 536 verdicts into a Python list costs milliseconds)"""
        ok = (C.c_int32 * max(nb, 1))()
        wrap = lambda b: b if isinstance(b, C.c_void_p) else _buf(b)     # noqa: E731
        self._ck(_lib.bpgpu_r1cs_verify_stream(self.ctx, gens, circuit, nb, n1, k, wrap(points), wrap(scalars), wrap(challenges), ok))
        return bytes(ok)[:4 * nb] if raw else ok[:nb]

    def r1cs_verify_screened_dev(self, gens, circuit, nb, n1, k, d_points, d_scalars, d_challenges, d_rho, d_ok):
        """combined check per batch first, per-proof path only for the batches that fail it (device-resident operands and verdicts;
        sync() before reading d_ok) -> number of batches that took the per-proof path"""
        nf = C.c_size_t(0)
        self._ck(_lib.bpgpu_r1cs_verify_screened_dev(self.ctx, gens, circuit, nb, n1, k, d_points, d_scalars, d_challenges, d_rho, d_ok, C.byref(nf)))
        return nf.value

    def r1cs_verify_screened_fs_dev(self, gens, circuit, nb, n1, k, d_init_states, d_points, d_scalars, d_rho, d_ok):
        """the same with the transcript replayed on the device (whole Verifier::verify; 1-phase circuits) -> fallback batches"""
        nf = C.c_size_t(0)
        self._ck(_lib.bpgpu_r1cs_verify_screened_fs_dev(self.ctx, gens, circuit, nb, n1, k, d_init_states, d_points, d_scalars, d_rho, d_ok,
                                                        C.byref(nf)))
        return nf.value

    def r1cs_verify_screened(self, gens, circuit, nb, n1, k, points, scalars, challenges, rho):
        """the same from host memory (bytes or c_void_p of page-locked memory) -> ([ok], fallback batches)"""
        ok = (C.c_int32 * max(nb, 1))()
        nf = C.c_size_t(0)
        wrap = lambda b: b if isinstance(b, C.c_void_p) else _buf(b)     # noqa: E731
        self._ck(_lib.bpgpu_r1cs_verify_screened(self.ctx, gens, circuit, nb, n1, k, wrap(points), wrap(scalars), wrap(challenges), wrap(rho), ok,
                                                 C.byref(nf)))
        return list(ok)[:nb], nf.value

    def r1cs_verify_batch_dev(self, gens, circuit, nb, n1, k, d_points, d_scalars, d_challenges, d_ok, d_mega=None,
                              d_full=None):
        self._ck(_lib.bpgpu_r1cs_verify_batch_dev(self.ctx, gens, circuit, nb, n1, k, d_points, d_scalars, d_challenges, d_ok, d_mega, d_full))


POOL_MAX_SLOTS = 32         # BPGPU_POOL_MAX_SLOTS


def pool_shares(nb, nslots, granule):
    """the split every pool call uses (bpgpu_pool_shares; needs no device): nslots + 1 bounds, share s = [lo[s], lo[s + 1])"""
    lo = (C.c_size_t * (nslots + 1))()
    rc = _lib.bpgpu_pool_shares(nb, nslots, granule, lo)
    if rc:
        raise BpGpuError(rc, _lib.bpgpu_strerror(rc).decode())
    return list(lo)


class BpPool:
    """Queues of independent proofs over several devices from one process (include/bpgpu.h, bpgpu_pool_*): one slot -- a context
    and a host thread -- per entry of `devices`; a device may appear several times.  Byte encodings and layouts as in BpGpu."""

    def __init__(self, devices=(0,)):
        self.pool = C.c_void_p()
        devs = (C.c_int * max(len(devices), 1))(*devices)
        rc = _lib.bpgpu_pool_create(devs, len(devices), C.byref(self.pool))
        if rc:
            raise BpGpuError(rc, _lib.bpgpu_strerror(rc).decode())

    def close(self):
        """(the pool's generators and circuits are destroyed before it)"""
        if self.pool:
            _lib.bpgpu_pool_destroy(self.pool)
            self.pool = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc:
            raise BpGpuError(rc, _lib.bpgpu_strerror(rc).decode() + " | " + _lib.bpgpu_pool_last_error(self.pool).decode())

    def slots(self):
        return _lib.bpgpu_pool_slots(self.pool)

    def device(self, slot):
        return _lib.bpgpu_pool_device(self.pool, slot)

    def ctx(self, slot):
        """the context of a slot as a BpGpu that does not own it (options, profiling, any single-context call)"""
        p = _lib.bpgpu_pool_ctx(self.pool, slot)
        if not p:
            raise BpGpuError(E_ARG, "bpgpu_pool_ctx: no such slot")
        return BpGpu.borrowed(p)

    def set_option(self, name, value):
        """bpgpu_set_option on every slot, all or nothing"""
        self._ck(_lib.bpgpu_pool_set_option(self.pool, OPT[name], int(value)))

    shares = staticmethod(pool_shares)

    # ---- handles: one per distinct device, shared by that device's slots
    def gens_create(self, G, H, B, B_blinding, window_bits=8):
        h = C.c_void_p()
        self._ck(_lib.bpgpu_pool_gens_create(self.pool, _buf(G), _buf(H), len(G) // 64, _buf(B), _buf(B_blinding), window_bits, C.byref(h)))
        return h

    def gens_destroy(self, h):
        _lib.bpgpu_pool_gens_destroy(self.pool, h)

    def gens_get(self, h, slot):
        """the bpgpu_gens of the slot's device (for single-context calls on ctx(slot)), as an address"""
        return _lib.bpgpu_pool_gens_get(h, slot)

    def circuit_create(self, row_ptr, kind, idx, coeff, n_mul, m, ark=False):
        q, nnz = len(row_ptr) - 1, len(kind)
        h = C.c_void_p()
        rp = (C.c_uint32 * (q + 1))(*row_ptr)
        kd = (C.c_uint32 * max(nnz, 1))(*kind)
        ix = (C.c_uint32 * max(nnz, 1))(*idx)
        fn = _lib.bpgpu_pool_circuit_create_ark if ark else _lib.bpgpu_pool_circuit_create
        self._ck(fn(self.pool, q, rp, kd, ix, _buf(coeff), n_mul, m, C.byref(h)))
        return h

    def circuit_destroy(self, h):
        _lib.bpgpu_pool_circuit_destroy(self.pool, h)

    def circuit_get(self, h, slot):
        return _lib.bpgpu_pool_circuit_get(h, slot)

    def circuit_create_param(self, q, nchi, row_ptr, kind, idx, coeff, n_mul, m):
        """BpGpu.circuit_create_param per distinct device: a handle that r1cs_prove_values takes (the other pool calls refuse it)"""
        h = C.c_void_p()
        self._ck(_lib.bpgpu_pool_circuit_create_param(self.pool, q, nchi, _u32s(row_ptr), _u32s(kind), _u32s(idx), _buf(coeff), n_mul, m,
                                                      C.byref(h)))
        return h

    def circuit_set_gadget_labels(self, circuit, labels):
        """BpGpu.circuit_set_gadget_labels on every slot's handle"""
        tab = None if labels is None else _buf(b"".join((bytes(x) + bytes(32))[:32] for x in labels))
        self._ck(_lib.bpgpu_pool_circuit_set_gadget_labels(self.pool, circuit, tab))

    def witness_create(self, n, n1, m, nchi, op, arg, row_ptr, kind, idx, coeff):
        """BpGpu.witness_create per distinct device"""
        h = C.c_void_p()
        self._ck(_lib.bpgpu_pool_witness_create(self.pool, n, n1, m, nchi, _buf(bytes(op)), _u32s(arg), _u32s(row_ptr), _u32s(kind), _u32s(idx),
                                                _buf(coeff), C.byref(h)))
        return h

    def witness_destroy(self, h):
        _lib.bpgpu_pool_witness_destroy(self.pool, h)

    def witness_get(self, h, slot):
        return _lib.bpgpu_pool_witness_get(h, slot)

    # ---- the four calls: operands for the whole queue as bytes, or c_void_p of page-locked memory
    @staticmethod
    def _wrap(b):
        return b if isinstance(b, C.c_void_p) else _buf(b)

    def r1cs_verify_stream(self, gens, circuit, nb, n1, k, points, scalars, challenges, want_shares=False, raw=False):
        """bpgpu_r1cs_verify_stream on every slot's share -> [ok] (raw: the nb x int32 verdicts as bytes); want_shares: (ok, proofs per slot)"""
        ok = (C.c_int32 * max(nb, 1))()
        per = (C.c_size_t * max(self.slots(), 1))()
        self._ck(_lib.bpgpu_pool_r1cs_verify_stream(self.pool, gens, circuit, nb, n1, k, self._wrap(points), self._wrap(scalars),
                                                    self._wrap(challenges), ok, per))
        out = bytes(ok)[:4 * nb] if raw else ok[:nb]
        return (out, list(per)) if want_shares else out

    def r1cs_verify_screened(self, gens, circuit, nb, n1, k, points, scalars, challenges, rho):
        """-> ([ok], fallback batches summed over the slots)"""
        ok = (C.c_int32 * max(nb, 1))()
        nf = C.c_size_t(0)
        self._ck(_lib.bpgpu_pool_r1cs_verify_screened(self.pool, gens, circuit, nb, n1, k, self._wrap(points), self._wrap(scalars),
                                                      self._wrap(challenges), self._wrap(rho), ok, C.byref(nf)))
        return list(ok)[:nb], nf.value

    def r1cs_verify_combined(self, gens, circuit, nb, n1, k, points, scalars, challenges, rho):
        """sum over the whole queue of rho_p * mega_check_p: the slots' partial points added on slot 0 (64 bytes; all zero: every proof valid)"""
        o = _out(64)
        self._ck(_lib.bpgpu_pool_r1cs_verify_combined(self.pool, gens, circuit, nb, n1, k, self._wrap(points), self._wrap(scalars),
                                                      self._wrap(challenges), self._wrap(rho), o))
        return bytes(o)

    def r1cs_prove_fs(self, gens, circuit, nb, n, m, states, a_L, a_R, a_O, blindings, v_blinding=None, s_L=None, s_R=None,
                      vector_keys=None, want_wire=True):
        """BpGpu.r1cs_prove_fs with the provers dealt over the slots: the same operands, the same five results"""
        k = max(n - 1, 0).bit_length()
        nvar, plen = 11 + 2 * k, 1 + 11 * 32 + (2 * k + 2) * 32
        pts, sc, ch, so = _out(64 * nb * nvar), _out(160 * nb), _out(32 * nb * (5 + k)), _out(32 * nb)
        wire = _out(nb * plen) if want_wire else None
        opt = lambda b: _buf(b) if b is not None else None     # noqa: E731
        self._ck(_lib.bpgpu_pool_r1cs_prove_fs(self.pool, gens, circuit, nb, opt(states), opt(a_L), opt(a_R), opt(a_O), opt(s_L), opt(s_R),
                                               opt(vector_keys), opt(v_blinding), opt(blindings), pts, sc, wire, ch, so))
        return (bytes(pts)[:64 * nb * nvar], bytes(sc)[:160 * nb], bytes(wire)[:nb * plen] if want_wire else None,
                bytes(ch)[:32 * nb * (5 + k)], bytes(so)[:32 * nb])

    def r1cs_prove_values(self, gens, circuit, w, nb, n, m, *, init_states, blindings, v=None, v_blinding=None, inputs=None,
                          gadget_label=None, s_L=None, s_R=None, vector_keys=None, want_wire=True, want_witness=False,
                          nchi=None):
        """BpGpu.r1cs_prove_values with the provers dealt over the slots (pool handles): the same operands -> ProveValues"""
        lab = _label(gadget_label)
        return _prove_values_host(lambda *a: self._ck(_lib.bpgpu_pool_r1cs_prove_values(self.pool, gens, circuit, w, *a)), nb, n, m, lab,
                                  init_states, v, v_blinding, inputs, s_L, s_R, vector_keys, blindings, want_wire, want_witness, nchi)
