"""Test side of the two-party prover calls (include/bpgpu.h, bpgpu_mpc_*): a dealer of authenticated shares and Beaver triples, the
opening of the parties' planes with its MAC check, and a driver that runs party 0 and party 1 call by call on two contexts, with the
Fiat-Shamir transcript (oracle/pymodel.py) fed with the opened values.  Test infrastructure: the network, the fabric and the MAC
check stand in for the host a real deployment has."""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import pymodel as pm   # noqa: E402

N = pm.N
RM = pow(2, 256, N)
RM_INV = pow(RM, -1, N)
KIND = {"L": 0, "R": 1, "O": 2, "V": 3, "1": 4}


def mont(v):
    """ark-ff Montgomery form: v * 2^256 mod n, 32 bytes little endian"""
    return (v % N * RM % N).to_bytes(32, "little")


def unmont(b):
    return int.from_bytes(b, "little") * RM_INV % N


def le(v):
    return (v % N).to_bytes(32, "little")


def cut(b, size):
    return [b[i:i + size] for i in range(0, len(b), size)]


class Dealer:
    """alpha = alpha_0 + alpha_1; a value v splits into (s_p, m_p, c) per party with v = s_0 + s_1 + c, m_0 + m_1 = alpha (s_0 + s_1)
    and a random non-zero public modifier c; triples carry a zero modifier"""

    def __init__(self, seed):
        self.rnd = random.Random(seed)
        self.alpha_sh = [self.rnd.randrange(N), self.rnd.randrange(N)]
        self.alpha = sum(self.alpha_sh) % N
        self.bad = []           # names of opened quantities whose MAC identity failed
        self.mod_mismatch = []  # names whose modifier planes differ between the parties

    def share(self, v, modifier=True):
        c = self.rnd.randrange(1, N) if modifier else 0
        s0 = self.rnd.randrange(N)
        s1 = (v - s0 - c) % N
        m0 = self.rnd.randrange(N)
        m1 = (self.alpha * (s0 + s1) - m0) % N
        return (s0, m0, c), (s1, m1, c)

    def share_vec(self, vals, modifier=True):
        """-> [party][plane][i]"""
        out = [[[], [], []], [[], [], []]]
        for v in vals:
            for p, sh in enumerate(self.share(v, modifier)):
                for k in range(3):
                    out[p][k].append(sh[k])
        return out

    def triples(self, count, bad=None):
        """count Beaver triples -> [party][t = x, y, z][plane][i]; bad: index whose z is not x y"""
        xs = [self.rnd.randrange(N) for _ in range(count)]
        ys = [self.rnd.randrange(N) for _ in range(count)]
        zs = [x * y % N for x, y in zip(xs, ys)]
        if bad is not None:
            zs[bad] = (zs[bad] + 1) % N
        sh = [self.share_vec(v, modifier=False) for v in (xs, ys, zs)]
        return [[sh[t][p] for t in range(3)] for p in range(2)]

    def open_sc(self, name, planes):
        """planes[p] = (s, m, c) -> the value; records a failed MAC identity / differing modifiers under `name`"""
        (s0, m0, c0), (s1, m1, c1) = planes
        if c0 != c1:
            self.mod_mismatch.append(name)
        if (m0 + m1) % N != self.alpha * (s0 + s1) % N:
            self.bad.append(name)
        return (s0 + s1 + c0) % N

    def open_pt(self, name, planes, check_mac=True):
        """planes[p] = (S, M, C) 64-byte points -> the opened point's bytes"""
        (S0, M0, C0), (S1, M1, C1) = [[pm.b2p(x) for x in q] for q in planes]
        if planes[0][2] != planes[1][2]:
            self.mod_mismatch.append(name)
        S = pm.pt_add(S0, S1)
        if check_mac and pm.pt_add(M0, M1) != pm.pt_mul(self.alpha, S):
            self.bad.append(name)
        return pm.p2b(pm.pt_add(S, C0))


def pack(rows):
    """nested lists of ints -> concatenated Montgomery bytes (depth-first)"""
    if isinstance(rows, int):
        return mont(rows)
    return b"".join(pack(r) for r in rows)


def circuit_rows(constraints, param=False, nchi=None):
    """CSR rows (row_ptr, kind, idx, coeff) of the model's constraints; param: the shuffle's (1 + 1) q rows with every `One` term
    -chi moved to the chi block as -1 (include/bpgpu.h bpgpu_circuit_create_param), and chi.
    A constraint is the model's dict, or a list of (var, coeff) terms kept as they are: repeated variables and zero coefficients
    stay separate terms.  nchi: the (1 + nchi) q rows of a circuit whose coefficients may be tuples (c0, c1, .., c_nchi) standing
    for c0 + sum_j chi_j c_j -- part j goes to block j, None parts to none (tests/circuit_gen.py)."""
    q = len(constraints)
    blocks = [[[] for _ in range(q)] for _ in range(1 + nchi if nchi is not None else (2 if param else 1))]
    chi = None
    for r, lc in enumerate(constraints):
        for var, c in (lc.items() if isinstance(lc, dict) else lc):
            if isinstance(c, tuple):
                for j, cj in enumerate(c):
                    if cj is not None:
                        blocks[j][r].append((KIND[var[0]], var[1] if len(var) > 1 else 0, cj % N))
            elif param and var[0] == "1":
                assert chi is None or chi == (-c) % N
                chi = (-c) % N
                blocks[1][r].append((4, 0, N - 1))
            else:
                blocks[0][r].append((KIND[var[0]], var[1] if len(var) > 1 else 0, c % N))
    rp, kd, ix, cf = [0], [], [], b""
    for b in blocks:
        for row in b:
            for k_, i_, c_ in row:
                kd.append(k_)
                ix.append(i_)
                cf += le(c_)
            rp.append(len(kd))
    return rp, kd, ix, cf, chi


def draw_blindings(seed, m, n1, n2):
    """the blinding values Prover.prove draws (oracle/pymodel.py), from a fresh SplitMix64(seed) after the m v_blindings"""
    rng = pm.SplitMix64(seed)
    for _ in range(m):
        rng.scalar()
    b = {"ib1": rng.scalar(), "ob1": rng.scalar(), "sb1": rng.scalar()}
    b["sL"] = [rng.scalar() for _ in range(n1)]
    b["sR"] = [rng.scalar() for _ in range(n1)]
    b["ib2"], b["ob2"], b["sb2"] = (rng.scalar(), rng.scalar(), rng.scalar()) if n2 else (0, 0, 0)
    b["sL"] += [rng.scalar() for _ in range(n2)]
    b["sR"] += [rng.scalar() for _ in range(n2)]
    b["tb"] = [rng.scalar() for _ in range(5)]
    return b


def poly6(x, c):
    acc = 0
    for v in reversed(c):
        acc = x * (v + acc) % N
    return acc


def run_two_party(gpus, gens, provers, blinds, dealer, make_circuits, tamper=None):
    """One proof per prover (a model Prover after its commitments and phase-1 gadget, oracle/pymodel.py) run as two parties, party p on
    gpus[p] with its generators gens[p].  make_circuits(provers) -> (circuit handle per party, gadget challenges bytes or None), called
    once the randomized constraints exist.  tamper: None, "share" (party 0's share of a_L[0] of proof 0), "mac" (its MAC share) or
    "triple" (one polynomial triple of proof 0 with z != x y).  Returns the opened proofs (dicts of bytes / ints as Prover.prove), the
    challenges and the shapes."""
    nb = len(provers)
    trs = [pv.transcript for pv in provers]
    m = len(provers[0].v)
    n1 = len(provers[0].a_L)
    for tr in trs:
        tr.append_u64(b"m", m)
    proofs = [dict() for _ in range(nb)]
    wit = []
    for p, pv in enumerate(provers):
        w = {key: dealer.share_vec(vals) for key, vals in (("aL", pv.a_L), ("aR", pv.a_R), ("aO", pv.a_O))}
        if tamper == "share" and p == 0:
            w["aL"][0][0][0] = (w["aL"][0][0][0] + 1) % N
        if tamper == "mac" and p == 0:
            w["aL"][0][1][0] = (w["aL"][0][1][0] + 1) % N
        b = blinds[p]
        w["sL"], w["sR"] = dealer.share_vec(b["sL"]), dealer.share_vec(b["sR"])
        for key in ("ib1", "ob1", "sb1", "ib2", "ob2", "sb2"):
            w[key] = dealer.share_vec([b[key]])
        w["tb"] = dealer.share_vec(b["tb"])
        w["vb"] = dealer.share_vec(pv.v_blinding)
        wit.append(w)

    def operands(party, lo, hi):
        return [pack([[wit[p][key][party][k][lo:hi] for k in range(3)] for p in range(nb)]) for key in ("aL", "aR", "aO", "sL", "sR")]

    def open_points(names, outs, per):
        for p in range(nb):
            for j, name in enumerate(names):
                planes = [[outs[q][((p * 3 + k) * per + j) * 64:((p * 3 + k) * per + j + 1) * 64] for k in range(3)] for q in range(2)]
                proofs[p][name] = dealer.open_pt("%s[%d]" % (name, p), planes)

    # phase 1 commitments, mpc_prover.rs:621-657
    sess, outs = [None, None], [None, None]
    for q in range(2):
        bl = pack([[[wit[p][key][q][k][0] for key in ("ib1", "ob1", "sb1")] for k in range(3)] for p in range(nb)])
        sess[q], outs[q] = gpus[q].mpc_prover_commit(gens[q], None, nb, n1, *operands(q, 0, n1), bl)
    open_points(["A_I1", "A_O1", "S1"], outs, 3)
    for p, tr in enumerate(trs):
        for name in ("A_I1", "A_O1", "S1"):
            tr.append_message(name.encode(), proofs[p][name])
    for pv in provers:
        pv._create_randomized_constraints()
    n = len(provers[0].a_L)
    n2 = n - n1
    padded = 1 if n == 0 else 1 << (n - 1).bit_length()
    if n2:   # the phase-2 multipliers' witness comes from the gadget (evaluating it on shares is the host's business)
        for p, pv in enumerate(provers):
            for key, vals in (("aL", pv.a_L), ("aR", pv.a_R), ("aO", pv.a_O)):
                sh = dealer.share_vec(vals[n1:])
                for q in range(2):
                    for k in range(3):
                        wit[p][key][q][k] += sh[q][k]
        for q in range(2):
            bl = pack([[[wit[p][key][q][k][0] for key in ("ib2", "ob2", "sb2")] for k in range(3)] for p in range(nb)])
            sess[q], outs[q] = gpus[q].mpc_prover_commit(gens[q], sess[q], nb, n2, *operands(q, n1, n), bl)
        open_points(["A_I2", "A_O2", "S2"], outs, 3)
    else:
        for p in range(nb):
            for name in ("A_I2", "A_O2", "S2"):
                proofs[p][name] = bytes(64)
    for p, tr in enumerate(trs):
        for name in ("A_I2", "A_O2", "S2"):
            tr.append_message(name.encode(), proofs[p][name])
    ch = [{"y": tr.challenge_scalar(b"y"), "z": tr.challenge_scalar(b"z")} for tr in trs]
    circs, chi = make_circuits(provers)
    # polynomials, mpc_prover.rs:783-829: six shared x shared products through triples
    trip = [[dealer.triples(n, bad=0 if (tamper == "triple" and p == 0 and j == 0) else None) for j in range(6)] for p in range(nb)]
    Y = b"".join(le(c["y"]) for c in ch)
    Z = b"".join(le(c["z"]) for c in ch)
    masked = [gpus[q].mpc_prover_polys_mask(sess[q], circs[q], nb, n, Y, Z, pack([[trip[p][j][q] for j in range(6)] for p in range(nb)]), chi)
              for q in range(2)]
    opened = b"".join(mont(dealer.open_sc("mask", [tuple(unmont(masked[q][((((p * 6 + j) * 2 + de) * 3 + k) * n + i) * 32:][:32])
                                                           for k in range(3)) for q in range(2)]))
                      for p in range(nb) for j in range(6) for de in range(2) for i in range(n))
    fin = [gpus[q].mpc_prover_polys_finish(sess[q], nb, m, opened, pack([[wit[p]["tb"][q][k] for k in range(3)] for p in range(nb)]))
           for q in range(2)]
    open_points(["T_1", "T_3", "T_4", "T_5", "T_6"], [f[1] for f in fin], 5)
    for p, tr in enumerate(trs):
        for name in ("T_1", "T_3", "T_4", "T_5", "T_6"):
            tr.append_message(name.encode(), proofs[p][name])
        ch[p]["u"] = tr.challenge_scalar(b"u")
        ch[p]["x"] = tr.challenge_scalar(b"x")
    # t_x, t_x_blinding, e_blinding: linear on the host, per plane (mpc_prover.rs:866-899)
    for p, tr in enumerate(trs):
        x, u = ch[p]["x"], ch[p]["u"]
        planes = {"t_x": [], "t_x_blinding": [], "e_blinding": []}
        for q in range(2):
            tq = [unmont(b) for b in cut(fin[q][0], 32)]
            wV = [int.from_bytes(b, "little") for b in cut(fin[q][2], 32)][p * m:(p + 1) * m]
            tx, txb, eb = [], [], []
            for k in range(3):
                t = tq[(p * 3 + k) * 6:(p * 3 + k + 1) * 6]
                tb = [wit[p]["tb"][q][k][i] for i in range(5)]
                tb2 = sum(c * vb for c, vb in zip(wV, wit[p]["vb"][q][k])) % N
                tx.append(poly6(x, t))
                txb.append(poly6(x, [tb[0], tb2] + tb[1:]))
                ib = (wit[p]["ib1"][q][k][0] + u * wit[p]["ib2"][q][k][0]) % N
                ob = (wit[p]["ob1"][q][k][0] + u * wit[p]["ob2"][q][k][0]) % N
                sb = (wit[p]["sb1"][q][k][0] + u * wit[p]["sb2"][q][k][0]) % N
                eb.append(x * (ib + x * (ob + x * sb)) % N)
            planes["t_x"].append(tuple(tx))
            planes["t_x_blinding"].append(tuple(txb))
            planes["e_blinding"].append(tuple(eb))
        for name in ("t_x", "t_x_blinding", "e_blinding"):
            proofs[p][name] = dealer.open_sc("%s[%d]" % (name, p), planes[name])
            tr.append_scalar(name.encode(), proofs[p][name])
        ch[p]["w"] = tr.challenge_scalar(b"w")
        tr.innerproduct_domain_sep(padded)
        proofs[p]["L_vec"], proofs[p]["R_vec"], ch[p]["us"] = [], [], []
    # the shared inner-product argument, mpc_inner_product.rs:52-228
    X, U, W = (b"".join(le(c[key]) for c in ch) for key in ("x", "u", "w"))
    ipp = [gpus[q].mpc_prover_ipp_begin(sess[q], gens[q], padded, n1, X, U, W) for q in range(2)]
    while gpus[0].ipp_len(ipp[0]) > 1:
        h = gpus[0].ipp_len(ipp[0]) // 2
        tr2 = [[dealer.triples(h) for _ in range(2)] for _ in range(nb)]
        masked = [gpus[q].mpc_ipp_mask(ipp[q], nb, pack([[tr2[p][j][q] for j in range(2)] for p in range(nb)])) for q in range(2)]
        opened = b"".join(mont(dealer.open_sc("ipp mask", [tuple(unmont(masked[q][((((p * 2 + j) * 2 + de) * 3 + k) * h + i) * 32:][:32])
                                                                   for k in range(3)) for q in range(2)]))
                          for p in range(nb) for j in range(2) for de in range(2) for i in range(h))
        lr = [gpus[q].mpc_ipp_round(ipp[q], nb, opened) for q in range(2)]
        us = b""
        for p, tr in enumerate(trs):
            for side, name in ((0, "L"), (1, "R")):
                planes = [[lr[q][side][(p * 3 + k) * 64:(p * 3 + k + 1) * 64] for k in range(3)] for q in range(2)]
                pt = dealer.open_pt("%s[%d]" % (name, p), planes)
                proofs[p][name + "_vec"].append(pt)
                tr.append_message(name.encode(), pt)
            u = tr.challenge_scalar(b"u")
            ch[p]["us"].append(u)
            us += le(u)
        uinv = b"".join(le(pow(int.from_bytes(c, "little"), -1, N)) for c in cut(us, 32))
        for q in range(2):
            gpus[q].ipp_fold(ipp[q], us, uinv)
    ab = [gpus[q].ipp_finish(ipp[q], 3 * nb) for q in range(2)]
    for p in range(nb):
        for side, name in ((0, "a"), (1, "b")):
            proofs[p][name] = dealer.open_sc("%s[%d]" % (name, p), [tuple(unmont(ab[q][side][(p * 3 + k) * 32:][:32]) for k in range(3))
                                                                    for q in range(2)])
    for q in range(2):
        gpus[q].ipp_destroy(ipp[q])
        gpus[q].prover_destroy(sess[q])
    return proofs, ch, dict(n1=n1, n=n, m=m, padded=padded, k=(padded - 1).bit_length(), circuits=circs, chi=chi)


def flat_proof(pr):
    """the CPU oracle's flat proof (oracle/bpo_api.c proof_to_flat) of an opened proof"""
    k = len(pr["L_vec"])
    out = k.to_bytes(4, "little") + bytes(4)
    for name in ("A_I1", "A_O1", "S1", "A_I2", "A_O2", "S2", "T_1", "T_3", "T_4", "T_5", "T_6"):
        out += pr[name]
    out += le(pr["t_x"]) + le(pr["t_x_blinding"]) + le(pr["e_blinding"])
    out += b"".join(pr["L_vec"]) + b"".join(pr["R_vec"]) + le(pr["a"]) + le(pr["b"])
    return out


def model_bytes(pr):
    """Prover.prove's proof dict with its points as 64-byte boundary encodings"""
    out = dict(pr)
    for name in ("A_I1", "A_O1", "S1", "A_I2", "A_O2", "S2", "T_1", "T_3", "T_4", "T_5", "T_6"):
        out[name] = pm.p2b(pr[name])
    out["L_vec"] = [pm.p2b(x) for x in pr["L_vec"]]
    out["R_vec"] = [pm.p2b(x) for x in pr["R_vec"]]
    return out
