"""tests/codec_cases.py against the Python model: the crafted x solve their cubics, the discrete logarithms have the digits the
patterns name, and the model's verdict on every encoding is the one its family intends.  No GPU."""
import codec_cases as cc
from codec_cases import P, pm


def test_no_pattern_was_skipped_and_every_x_solves_its_cubic():
    b = cc.build()
    assert b.skipped == ()
    names = {c.name.rsplit("/", 1)[0] for c in b.cases if c.family == "digits"}
    assert names == {n for n, _ in cc.digit_patterns()} and len(names) == 9 + 6 * 4 + 15 * 2
    for c in b.cases:
        x = int.from_bytes(c.enc[:31] + bytes([c.enc[31] & 0x3F]), "little")
        if c.a is None:
            assert x >= P and c.kind == "noncanonical"
        else:
            assert x < P and cc.rhs(x) == c.a, c.name
    # three encodings per digit pattern: both sign flags and the identity flag
    assert sum(c.family == "digits" for c in b.cases) == 3 * len(names)


def test_discrete_logarithm_digits_are_the_patterns():
    b = cc.build()
    pats = dict(cc.digit_patterns())
    odd = even = 0
    for fam, name, a in b.sqrt_args:
        if fam != "digits":
            continue
        e1 = pats[name]
        assert pow(a, cc.T, P) == pow(cc.C_GEN, e1, P), name
        assert (pm.fp_sqrt(a) is None) == bool(e1 & 1), name
        odd, even = odd + (e1 & 1), even + 1 - (e1 & 1)
    assert odd >= 10 and even >= 10
    assert cc.digits_of(pats["single_01_at_12"]) == [0] * 12 + [1] + [0] * 11
    assert cc.digits_of(pats["ff_below_3"]) == [0xFF] * 3 + [0] * 21 and cc.digits_of(pats["ff_from_3"]) == [0] * 3 + [0xFF] * 21
    assert cc.digits_of(pats["0100_repeated"])[:4] == [0, 1, 0, 1] and cc.digits_of(pats["00ff_repeated"])[:2] == [0xFF, 0]


def test_model_verdicts_are_the_intended_ones():
    b = cc.build()
    n_ok = n_bad = 0
    for c in b.cases:
        ok, xy = cc.model_decode(c.enc)
        assert ok == (1 if c.kind in ("valid", "identity") else 0), c.name
        if c.kind != "valid":
            assert xy == bytes(64), c.name
        else:
            assert xy != bytes(64) and pm.on_curve(pm.b2p(xy)), c.name
        n_ok, n_bad = n_ok + ok, n_bad + 1 - ok
    assert n_ok >= 20 and n_bad >= 20
    for kind in ("valid", "identity", "nonresidue", "noncanonical"):
        assert any(c.kind == kind for c in b.cases), kind
    # flags 01 mean the identity whatever x < p is; both flags, or x >= p, are refused whatever else holds
    assert cc.model_decode(cc.encode(P - 1, "01")) == (1, bytes(64))
    assert cc.model_decode(cc.encode(P - 1, "11")) == (0, bytes(64)) and cc.model_decode(cc.encode(P, "01")) == (0, bytes(64))


def test_valid_encodings_round_trip_in_the_model():
    b = cc.build()
    n = 0
    for c in b.cases:
        if c.kind == "valid":
            assert pm.point_compress(pm.point_decompress(c.enc)) == c.enc, c.name
            n += 1
    assert n >= 20


def test_sign_and_x_boundaries():
    b = cc.build()
    half = (P - 1) // 2
    ys = {y for _, y in b.sign_points}
    assert ys == {half - 1, half + 2, 2, P - 2}
    # no curve point has y = (p - 1) / 2, (p + 1) / 2, 1 or p - 1 (the offsets build() asserts), so these are the nearest
    for x, y in b.sign_points:
        assert pm.on_curve((x, y))
        assert (pm.point_compress((x, y))[31] >> 7) == (1 if y > half else 0)
        # either flag decodes: to this point or to its negative
        assert {pm.point_decompress(cc.encode(x, fl)) for fl in ("00", "10")} == {(x, y), (x, P - y)}
    assert {x for x, _ in b.x_points} == {1, 2, P - 2, P - 1} and all(pm.on_curve(pt) for pt in b.x_points)
    assert pm.fp_sqrt(cc.rhs(0)) is None and pm.fp_sqrt(cc.rhs(P - 3)) is None


def test_summary_counts():
    s = cc.summary()
    assert s["digits"][0] == 189 and s["digits"][2] == 63
    assert s["sign"][0] == s["sign"][1] and s["sign"][2] == s["sign"][3] == 4
    assert all(0 < v[1] < v[0] and 0 < v[3] < v[2] for f, v in s.items() if f != "sign")
