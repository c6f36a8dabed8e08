"""Seeded generator of R1CS circuits for the tests: the shapes the four gadgets of the oracle never have -- long and ragged columns,
coefficients at the edges of the field, a variable several times in one row, explicit zeros, empty rows, unused variables, constants
in some rows only, and second-phase rows whose coefficients are affine in up to eight gadget challenges.

A circuit is a list of rows; a row is a list of (var, coeff) terms in which a variable may repeat (the reference's
LinearCombination is a Vec).  var is the model's ('L' | 'R' | 'O' | 'V', i) or ('1',) (oracle/pymodel.py); coeff is an integer, or
for a second-phase row of a parametric circuit a tuple (c0, c1, .., c_nchi) that stands for c0 + sum_j chi_j c_j, where None means
"no term in that block" and 0 an explicit zero term.  Rows [0, q1) are first-phase constraints over the n1 first-phase multipliers
and the m committed values; rows [q1, q) are added by specify_randomized_constraints together with the n2 second-phase multipliers.
Every circuit comes with a witness that satisfies it for every value of the gadget challenges: a row's constant (or, where the row
has none, one balancing term) is minus the evaluation of the rest, block by block.

Pure Python on the model's integers; the CSR arrays come from mpc_dealer.circuit_rows."""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import pymodel as pm          # noqa: E402
import mpc_dealer as md       # noqa: E402

N = pm.N
ONE = pm.ONE
COLUMN_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 48, 257)     # around the lazy sums' reduction every 16th term, and one long column
EDGE_COEFFS = (0, 1, N - 1, N - 2, 1 << 251, (N + 1) // 2)
PROFILES = ("sparse", "dense", "columns", "edge_coeff", "dups", "holes")
CHI_LABEL = b"generated gadget challenge"


def _blocks(c, nchi):
    """a coefficient as its 1 + nchi block parts (None: absent)"""
    return tuple(c) if isinstance(c, tuple) else (c,) + (None,) * nchi


def coeff_at(c, chi):
    """the value of a coefficient for the gadget challenges chi"""
    if not isinstance(c, tuple):
        return c % N
    return ((c[0] or 0) + sum(x * (cj or 0) for x, cj in zip(chi, c[1:]))) % N


class Circuit:
    def __init__(self, seed, n1, n2, m, q, nchi=0, profile="sparse"):
        prof = set(profile.split("+"))
        assert prof <= set(PROFILES) and 0 <= nchi <= 8, profile
        self.seed, self.n1, self.n2, self.n, self.m, self.q, self.nchi, self.profile = seed, n1, n2, n1 + n2, m, q, nchi, profile
        two_phase = n2 > 0 or nchi > 0
        self.q1 = q // 2 if two_phase else q
        self.two_phase = two_phase
        rnd = random.Random(seed)
        n, q1 = self.n, self.q1
        # ---- the witness
        self.a_L = [rnd.randrange(1, N) for _ in range(n)]
        self.a_R = [rnd.randrange(1, N) for _ in range(n)]
        self.v = [rnd.randrange(1, N) for _ in range(m)]
        val = {ONE: 1}
        for i in range(n):
            val[("L", i)], val[("R", i)], val[("O", i)] = self.a_L[i], self.a_R[i], self.a_L[i] * self.a_R[i] % N
        for i in range(m):
            val[("V", i)] = self.v[i]
        # ---- which variables and rows take part
        vars1 = [(k, i) for k in "LRO" for i in range(n1)] + [("V", i) for i in range(m)]
        vars2 = vars1 + [(k, i) for k in "LRO" for i in range(n1, n)]
        unused, empty = set(), set()
        if "holes" in prof:
            if n >= 2:
                i = rnd.randrange(n)
                unused |= {("L", i), ("R", i), ("O", i)}
            if m >= 2:
                unused.add(("V", rnd.randrange(m)))
            empty = {0, q - 1} | {r for r in range(q) if rnd.random() < 0.1}
        self.unused, self.empty = unused, empty
        live = [r for r in range(q) if r not in empty]

        def eligible(var):
            return [r for r in live if r >= q1] if var[0] != "V" and var[1] >= n1 else live

        def fit(length, rows):
            return length if length <= len(rows) else max(x for x in COLUMN_LENGTHS if x <= len(rows))

        # ---- `columns`: chosen variables get a column of an exact length (the last first-phase multiplier stays free: it balances
        # the rows that have no constant)
        chosen = {}
        if "columns" in prof:
            for ki, k in enumerate("LROV"):
                cnt = m if k == "V" else n
                for i in range(min(cnt, len(COLUMN_LENGTHS))):
                    var = (k, i)
                    if var in unused or (k != "V" and n1 >= 2 and i == n1 - 1):
                        continue
                    chosen[var] = fit(COLUMN_LENGTHS[(i + 3 * ki) % len(COLUMN_LENGTHS)], eligible(var))
        self.column_lengths = dict(chosen)
        free1 = [x for x in vars1 if x not in unused and x not in chosen]
        free2 = [x for x in vars2 if x not in unused and x not in chosen]
        base = "dense" if "dense" in prof else ("sparse" if "sparse" in prof or "columns" not in prof else None)
        edge = "edge_coeff" in prof
        uniform = {var: EDGE_COEFFS[1 + j % 5] for j, var in enumerate(chosen) if edge and j % 2 == 0}

        def draw():
            if edge:
                return rnd.choice(EDGE_COEFFS + (rnd.randrange(N),))
            return rnd.choice((1, N - 1, rnd.randrange(1, N)))

        def coeff(var, r):
            c = uniform[var] if var in uniform else draw()
            if not nchi or r < q1:
                return c
            if var in chosen:              # one CSR term: the column keeps its exact length
                j = rnd.randrange(1 + nchi)
                return tuple(c if t == j else None for t in range(1 + nchi))
            parts = [None if rnd.random() < 0.2 else c] + [draw() if rnd.random() < 0.5 else None for _ in range(nchi)]
            if all(x is None for x in parts):
                parts[0] = c
            return tuple(parts)

        rows = [[] for _ in range(q)]
        for r in live:
            pool = free1 if r < q1 else free2
            if base == "dense":
                rows[r] = [(var, coeff(var, r)) for var in pool]
            elif base == "sparse" and pool:
                rows[r] = [(var, coeff(var, r)) for var in rnd.sample(pool, min(len(pool), rnd.randint(1, 3)))]
        for var, length in chosen.items():
            for r in rnd.sample(eligible(var), length):
                rows[r].append((var, coeff(var, r)))
        # ---- `dups`: a term split into 2-4 terms of the same variable, and a group of terms of one variable that sums to zero
        if "dups" in prof:
            first = True
            for r in live:
                pool = free1 if r < q1 else free2
                cand = [t for t, (var, _) in enumerate(rows[r]) if var not in chosen]
                if cand and (first or rnd.random() < 0.5):
                    t = rnd.choice(cand)
                    var, c = rows[r][t]
                    rows[r][t:t + 1] = [(var, p) for p in self._split(rnd, c, rnd.randint(2, 4))]
                if pool and (first or rnd.random() < 0.3):
                    var = rnd.choice(pool)
                    zero = 0 if not nchi or r < q1 else (0,) + tuple(rnd.choice((0, None)) for _ in range(nchi))
                    for p in self._split(rnd, zero, rnd.randint(2, 4)):
                        rows[r].insert(rnd.randint(0, len(rows[r])), (var, p))
                first = False
        # ---- constants: every live row, or some only (`holes`), or a column of an exact length (`columns`)
        if "columns" in prof:
            const_rows = set(rnd.sample(live, fit(COLUMN_LENGTHS[seed % len(COLUMN_LENGTHS)], live)))
            self.column_lengths[ONE] = len(const_rows)
        elif "holes" in prof:
            const_rows = {r for r in live if rnd.random() < 0.5}
        else:
            const_rows = set(live)
        # ---- make the witness satisfy every row, block by block
        for r in live:
            row = rows[r]
            if r in const_rows:
                row.append((ONE, 0))
                t = len(row) - 1
            elif not row:
                continue
            else:
                pool = free1 if r < q1 else free2
                if pool:
                    row.append((rnd.choice(pool), 0))
                t = len(row) - 1
            nb = 1 + (nchi if r >= q1 else 0)
            rest = [0] * nb
            for s, (var, c) in enumerate(row):
                if s != t:
                    for j, cj in enumerate(_blocks(c, nb - 1)):
                        rest[j] += (cj or 0) * val[var]
            var = row[t][0]
            fix = [(-x) * pow(val[var], -1, N) % N for x in rest]
            if nb == 1:
                row[t] = (var, fix[0])
            else:                          # chi blocks that need no balance stay without a term
                row[t] = (var, (fix[0],) + tuple(x if x else None for x in fix[1:]))
        self.rows = rows

    @staticmethod
    def _split(rnd, c, k):
        """k coefficients that sum to c (block by block for an affine one)"""
        if isinstance(c, tuple):
            cols = [[None] * k if cj is None else Circuit._split(rnd, cj, k) for cj in c]
            return [tuple(col[i] for col in cols) for i in range(k)]
        parts = [rnd.randrange(N) for _ in range(k - 1)]
        return parts + [(c - sum(parts)) % N]

    # ---- descriptions
    def rows_at(self, chi=()):
        """the numeric rows for the gadget challenges chi"""
        return [[(var, coeff_at(c, chi)) for var, c in row] for row in self.rows]

    def broken(self):
        """the same circuit with one constant moved by one: the witness no longer satisfies it"""
        import copy
        other = copy.copy(self)
        other.rows = [list(row) for row in self.rows]
        for r, row in enumerate(other.rows):
            for t, (var, c) in enumerate(row):
                if var == ONE:
                    row[t] = (var, ((c[0] + 1) % N,) + c[1:]) if isinstance(c, tuple) else (var, (c + 1) % N)
                    return other
        raise ValueError("the circuit has no constant")

    def csr(self, ark=False):
        """(row_ptr, kind, idx, coeff bytes) of a numeric circuit for circuit_create; ark: coefficients in ark-ff Montgomery form"""
        assert self.nchi == 0
        rp, kd, ix, cf, _ = md.circuit_rows(self.rows)
        if ark:
            cf = b"".join(md.mont(int.from_bytes(cf[i:i + 32], "little")) for i in range(0, len(cf), 32))
        return rp, kd, ix, cf

    def csr_param(self):
        """(row_ptr, kind, idx, coeff bytes) of the (1 + nchi) q rows in block layout for circuit_create_param"""
        rp, kd, ix, cf, _ = md.circuit_rows(self.rows, nchi=self.nchi)
        return rp, kd, ix, cf

    # ---- the model
    def install(self, cs, rng=None, commitments=None, chi=None):
        """Put the circuit into a pm.Prover (with the witness; blindings of the commitments from rng) or a pm.Verifier (with the
        commitments).  Second-phase rows and multipliers go in through specify_randomized_constraints, which draws nchi challenges
        from the transcript; chi replaces their values (the transcript still advances).  Returns a dict: V the commitments, chi the
        challenges used (filled when the randomized constraints are created: prove / verify / _create_randomized_constraints)."""
        prover = isinstance(cs, pm.Prover)
        info = {"V": [], "chi": None if self.two_phase else []}
        for i in range(self.m):
            if prover:
                info["V"].append(cs.commit(self.v[i], rng.scalar())[0])
            else:
                cs.commit(commitments[i])
                info["V"].append(commitments[i])

        def multipliers(lo, hi):
            for i in range(lo, hi):
                cs.allocate_multiplier((self.a_L[i], self.a_R[i]) if prover else None)

        multipliers(0, self.n1)
        for row in self.rows[:self.q1]:
            cs.constrain(pm.lc(*row))
        if self.two_phase:
            def phase2(cs2):
                drawn = [cs2.challenge_scalar(CHI_LABEL) for _ in range(self.nchi)]
                info["chi"] = list(chi) if chi is not None else drawn
                multipliers(self.n1, self.n)
                for row in self.rows[self.q1:]:
                    cs2.constrain(pm.lc(*[(var, coeff_at(c, info["chi"])) for var, c in row]))
            cs.specify_randomized_constraints(phase2)
        return info


LABEL = b"GeneratedCircuit"


def prove(circ, bp_gens, seed=1):
    """pm.Prover.prove on the circuit and its witness -> (proof, install info with the commitments and the gadget challenges)"""
    pv = pm.Prover(pm.PedersenGens(), pm.Transcript(LABEL))
    rng = pm.SplitMix64(seed)
    info = circ.install(pv, rng=rng)
    return pv.prove(bp_gens, rng), info


def verifier(circ, commitments, chi=None):
    """a pm.Verifier holding the circuit -> (verifier, install info)"""
    vf = pm.Verifier(pm.PedersenGens(), pm.Transcript(LABEL))
    return vf, circ.install(vf, commitments=commitments, chi=chi)


def model_weights(circ, z, chi=None):
    """pm.Verifier.flattened_constraints(z) of the circuit (for the gadget challenges chi): wL, wR, wO, wV, wc"""
    vf, _ = verifier(circ, [pm.G] * circ.m, chi=chi)
    vf._create_randomized_constraints()
    assert vf.num_vars == circ.n and len(vf.constraints) == circ.q
    return vf.flattened_constraints(z)
