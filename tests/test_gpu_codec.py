"""GPU: the point codec (uzk_*_decompress_batch, uzk_*_compress_batch, the key-level decoders, uzk_test_sqrt_kat) against
tests/codec_ref.py, the restatement on Python integers, and against the project's earlier Python decoders.

The square roots are checked by squaring what comes back, squares and non-squares side by side in one wave.  Encodings of the key come
from tests/golden (the three parts of the reference's groth16_pk.bin); reference decodings are computed once per module and shared."""
import random

import numpy as np
import pytest

import codec_ref as cr
import ed_ref as ed
import g2_ref as g2

pytestmark = pytest.mark.gpu
P, Q = cr.P, cr.Q
_rng = random.Random("gpu-codec")
RHO = pow(5, (Q - 1) >> 28, Q)                                      # a primitive 2^28-th root of unity of Fr


def fq_wire(vals):
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        m = (v << 256) % P
        out[i] = [(m >> (64 * k)) & (2 ** 64 - 1) for k in range(4)]
    return out


def fq_unwire(a):
    inv = pow(1 << 256, -1, P)
    return [sum(int(r[k]) << (64 * k) for k in range(4)) * inv % P for r in np.asarray(a, dtype=np.uint64).reshape(-1, 4)]


def g1_points(wire):
    v = fq_unwire(wire)
    return [None if v[2 * i] == 0 and v[2 * i + 1] == 0 else (v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]


def g2_points(wire):
    v = fq_unwire(wire)
    return [None if not any(v[4 * i:4 * i + 4]) else ((v[4 * i], v[4 * i + 1]), (v[4 * i + 2], v[4 * i + 3])) for i in range(len(v) // 4)]


@pytest.fixture(scope="module")
def codec(gpu):
    from uzkge_amd import codec as c
    return c


@pytest.fixture(scope="module")
def key():
    data = cr.key_bytes()
    return data, cr.key_layout(data)


# ---- the square roots -------------------------------------------------------------------------------------------------------------------
def test_sqrt_fq(codec):
    sq = _rng.randrange(2, P) ** 2 % P
    nsq = next(v for v in iter(lambda: _rng.randrange(2, P), None) if pow(v, (P - 1) // 2, P) != 1)
    vals = [0, 1, P - 1, sq, nsq]
    vals += [v % P for k in range(1, 9) for v in ((1 << 29 * k) - 1, 1 << 29 * k, (1 << 29 * k) + 1)]         # limb boundaries
    vals += [v % P for k in range(1, 8) for v in ((1 << 32 * k) - 1, 1 << 32 * k)]                           # word boundaries
    vals += [_rng.randrange(P) for _ in range(64)]
    root, ok = codec.sqrt_kat(0, fq_wire(vals))
    for a, r, o in zip(vals, fq_unwire(root), ok):
        assert bool(o) == (a == 0 or pow(a, (P - 1) // 2, P) == 1), hex(a)
        assert not o or r * r % P == a, hex(a)


def test_sqrt_fq2(codec):
    s = _rng.randrange(2, P) ** 2 % P
    t = next(v for v in iter(lambda: _rng.randrange(2, P), None) if pow(v, (P - 1) // 2, P) != 1)
    vals = [(s, 0), (t, 0), (0, s), (0, t), (0, 0), (1, 0), (P - 1, 0), (0, 1), (0, P - 1)]
    squares, others = [], []
    while len(squares) < 64 or len(others) < 64:
        a = (_rng.randrange(P), _rng.randrange(1, P))
        (squares if g2.f2_sqrt(a) is not None else others).append(a)
    mixed = [v for pair in zip(squares[:64], others[:64]) for v in pair]              # side by side in the wave
    vals += mixed
    root, ok = codec.sqrt_kat(1, np.stack([fq_wire(list(a)).reshape(8) for a in vals]))
    r = fq_unwire(root)
    for i, a in enumerate(vals):
        want = g2.f2_sqrt(a) is not None
        assert bool(ok[i]) == want, a
        if want:
            x = (r[2 * i], r[2 * i + 1])
            assert g2.f2_sqr(x) == a, a
    assert fq_unwire(root[1])[0] == 0                                                 # sqrt of a non-square of Fq lies on the u axis
    assert [bool(o) for o in ok[:9]] == [True] * 9                                    # every element of Fq is a square in Fq2


def test_sqrt_fr(codec):
    vals, want = [0], [True]
    for k in range(28):                                                               # the 2-power part has order exactly 2^k
        for _ in range(2):
            v = _rng.randrange(1, Q)
            vals.append(pow(RHO, 1 << (28 - k), Q) * pow(v, 1 << 28, Q) % Q)
            want.append(True)
            vals.append(RHO * pow(_rng.randrange(1, Q), 1 << 28, Q) % Q)              # a non-square next to it
            want.append(False)
    vals += [1, Q - 1, 4, 5]
    want += [True, True, True, False]
    for _ in range(32):
        v = _rng.randrange(Q)
        vals.append(v)
        want.append(v == 0 or pow(v, (Q - 1) // 2, Q) == 1)
    for k in range(28):
        a = vals[1 + 4 * k]
        assert pow(a, ((Q - 1) >> 28) << k, Q) == 1 and (k == 0 or pow(a, ((Q - 1) >> 28) << (k - 1), Q) != 1)
    root, ok = codec.sqrt_kat(2, ed.fr_wire(vals))
    for a, r, o, w in zip(vals, ed.fr_unwire(root), ok, want):
        assert bool(o) == w, hex(a)
        assert not w or r * r % Q == a, hex(a)


# ---- batches ----------------------------------------------------------------------------------------------------------------------------
def _g1_bad():
    x = next(v for v in range(2, 100) if g2.fq_sqrt((v ** 3 + 3) % P) is None)
    return {"x = p": P.to_bytes(32, "little"), "x = p + 1": (P + 1).to_bytes(32, "little"), "x = 2^254 - 1": ((1 << 254) - 1).to_bytes(32, "little"),
            "both flags": bytes(31) + b"\xc0", "infinity with a body": b"\x01" + bytes(30) + b"\x40", "infinity with a high body": bytes(31) + b"\x41",
            "no point": x.to_bytes(32, "little"), "no point, sign": (x | 1 << 255).to_bytes(32, "little")}


def _g2_bad():
    x = next((v, 1) for v in range(2, 100) if g2.f2_sqrt(g2.f2_add(g2.f2_mul(g2.f2_sqr((v, 1)), (v, 1)), g2.B2)) is None)
    le = lambda v: v.to_bytes(32, "little")
    return {"x.c0 = p": le(P) + le(1), "x.c1 = p": le(1) + le(P), "x.c1 = p + 1": le(1) + le(P + 1), "x.c0 = 2^256 - 1": b"\xff" * 32 + le(1),
            "both flags": bytes(63) + b"\xc0", "infinity with c0": b"\x01" + bytes(62) + b"\x40", "infinity with c1": bytes(32) + b"\x01" + bytes(30) + b"\x40",
            "no point": le(x[0]) + le(x[1]), "no point, sign": le(x[0]) + le(x[1] | 1 << 255)}


def _ed_bad():
    y = next(v for v in range(2, 100) if cr.ed_decompress(v.to_bytes(32, "little"))[0] == cr.NO_POINT)
    le = lambda v: v.to_bytes(32, "little")
    return {"y = q": le(Q), "y = q + 1": le(Q + 1), "bit 254": le(1 << 254 | 5), "sign on (0, 1)": le(1 | 1 << 255), "sign on (0, q - 1)": le(Q - 1 | 1 << 255),
            "no point": le(y), "no point, sign": le(y | 1 << 255)}


@pytest.mark.parametrize("group", ["g1", "g2", "ed"])
def test_every_strictness_rule(codec, group):
    """One encoding per rule.  A sign bit on a y that is its own negation has no G1 or G2 instance: neither curve has a point with
    y = 0 (both groups have odd order), so that rule is exercised on the Edwards curve, where x = 0 has the points (0, 1) and (0, -1)."""
    bad = {"g1": _g1_bad, "g2": _g2_bad, "ed": _ed_bad}[group]()
    dec = {"g1": codec.g1_decompress, "g2": codec.g2_decompress, "ed": codec.ed_decompress}[group]
    ref = {"g1": cr.g1_decompress, "g2": cr.g2_decompress, "ed": cr.ed_decompress}[group]
    pts, st = dec(b"".join(bad.values()))
    want = [ref(e)[0] for e in bad.values()]
    assert all(want) and {1, 2} <= set(want)
    assert [int(s) for s in st] == want, list(zip(bad, st, want))
    assert not pts.any()


def test_g2_outside_the_subgroup(codec):
    q = cr.g2_outside_subgroup()
    good = cr.section_encodings(*_key_cache(), "b_g2_query")[1]
    enc = cr.g2_compress(q) + good + cr.g2_compress(g2.g2_neg(q)) + cr.g2_compress(None)
    pts, st = codec.g2_decompress(enc, check_subgroup=False)
    assert [int(s) for s in st] == [0, 0, 0, 0] and g2_points(pts) == [q, cr.g2_decompress(good)[1], g2.g2_neg(q), None]
    pts, st = codec.g2_decompress(enc, check_subgroup=True)
    assert [int(s) for s in st] == [3, 0, 3, 0] and g2_points(pts) == [None, cr.g2_decompress(good)[1], None, None]


def test_edwards_special_points(codec):
    o8 = ed.order8_point()
    pts = [(0, 1), (0, Q - 1), (1, 0), (Q - 1, 0), o8, ed.neg(o8), ed.G]
    enc = b"".join(cr.ed_compress(p) for p in pts)
    wire, st = codec.ed_decompress(enc, check_subgroup=False)
    assert [int(s) for s in st] == [0] * 7 and ed.points_unwire(wire) == pts
    wire, st = codec.ed_decompress(enc, check_subgroup=True)
    assert [int(s) for s in st] == [0, 3, 3, 3, 3, 3, 0] == [3 if ed.classify(p) else 0 for p in pts]
    assert ed.points_unwire(wire) == [pts[0]] + [(0, 0)] * 5 + [ed.G]
    back, st = codec.ed_compress(ed.points_wire(pts))
    assert not st.any() and b"".join(bytes(r) for r in back) == enc


_kc = []


def _key_cache():
    if not _kc:
        data = cr.key_bytes()
        _kc.extend([data, cr.key_layout(data)])
    return _kc


def _mixed(good, bad, n):
    """n encodings: good ones (infinities among them) with a bad one at every fifth place, the first and the last lane"""
    out = []
    for i in range(n):
        out.append(bad[i % len(bad)] if (i % 5 == 2 or i in (0, n - 1)) and n > 1 else good[i % len(good)])
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 100, 257])
def test_batch_edges(codec, n):
    """one lane, around a wave, a size that is no multiple of the block, several blocks: good, infinite and bad encodings interleaved"""
    data, layout = _key_cache()
    g1_good = cr.section_encodings(data, layout, "a_query")[:40]
    g2_good = cr.section_encodings(data, layout, "b_g2_query")[:40]
    assert any(e[-1] & 0x40 for e in g1_good) and any(e[-1] & 0x40 for e in g2_good)
    ed_good = [cr.ed_compress(p) for p in ed.rand_subgroup_points(12, 5)] + [cr.ed_compress(ed.order8_point())]
    for good, bad, dec, enc, ref, unwire in ((g1_good, list(_g1_bad().values()), codec.g1_decompress, codec.g1_compress, _ref_g1, g1_points),
                                             (g2_good, list(_g2_bad().values()), codec.g2_decompress, codec.g2_compress, _ref_g2, g2_points),
                                             (ed_good, list(_ed_bad().values()), codec.ed_decompress, codec.ed_compress, _ref_ed, None)):
        encs = _mixed(good, bad, n)
        pts, st = dec(b"".join(encs))
        want = [ref(e) for e in encs]
        assert [int(s) for s in st] == [w[0] for w in want]
        if unwire:
            assert unwire(pts) == [w[1] for w in want]
        else:
            assert ed.points_unwire(pts) == [w[1] if w[0] == 0 else (0, 0) for w in want]
        ok = [i for i in range(n) if st[i] == 0]
        if ok:
            back, st2 = enc(pts[ok])
            assert not st2.any() and [bytes(r) for r in back] == [encs[i] for i in ok]


_memo = {}


def _memoized(fn, e):
    if (fn, e) not in _memo:
        _memo[(fn, e)] = fn(e)
    return _memo[(fn, e)]


def _ref_g1(e): return _memoized(cr.g1_decompress, e)
def _ref_g2(e): return _memoized(cr.g2_decompress, e)
def _ref_ed(e): return _memoized(cr.ed_decompress, e)


def test_compress_refuses_words_at_or_above_the_modulus(codec):
    good = g2.points_to_wire([cr.g2_decompress(cr.section_encodings(*_key_cache(), "beta_g2")[0])[1]])[0]
    raw = lambda v: [(v >> (64 * k)) & (2 ** 64 - 1) for k in range(4)]
    g1w = np.array([raw(P) + raw(1), raw(1) + raw(P + 5), raw(0) + raw(0)], dtype=np.uint64)
    enc, st = codec.g1_compress(g1w)
    assert [int(s) for s in st] == [1, 1, 0] and bytes(enc[2]) == cr.g1_compress(None) and not enc[:2].any()
    g2w = np.stack([good, good, np.zeros(16, dtype=np.uint64)])
    g2w[1, 12:16] = raw(P)
    enc, st = codec.g2_compress(g2w)
    assert [int(s) for s in st] == [0, 1, 0] and bytes(enc[0]) == cr.section_encodings(*_key_cache(), "beta_g2")[0] and bytes(enc[2]) == cr.g2_compress(None)
    edw = np.array([raw(Q) + raw(1), raw(0) + raw(2 ** 256 - 1)], dtype=np.uint64)
    enc, st = codec.ed_compress(edw)
    assert [int(s) for s in st] == [1, 1] and not enc.any()


# ---- the whole key ----------------------------------------------------------------------------------------------------------------------
def _sample(encodings, limit=2048):
    """the first, the last and every infinity's neighbours, always; then random others up to `limit` points in all (a_query's 2046
    infinities have more neighbours than that: there the neighbours are the sample)"""
    n = len(encodings)
    idx = {0, n - 1}
    for i, e in enumerate(encodings):
        if e[-1] & 0x40:
            idx |= {max(i - 1, 0), min(i + 1, n - 1)}
    rest = [i for i in range(n) if i not in idx]
    random.Random(n).shuffle(rest)
    return sorted(idx) + rest[:max(0, limit - len(idx))]


@pytest.mark.parametrize("name", cr.SECTIONS)
def test_whole_key_section(gpu, codec, key, name):
    data, layout = key
    encs = cr.section_encodings(data, layout, name)
    is_g2 = name in cr.G2_SECTIONS
    pts, st = (codec.g2_decompress if is_g2 else codec.g1_decompress)(b"".join(encs))
    assert not st.any()
    inf = [bool(e[-1] & 0x40) for e in encs]
    assert [not row.any() for row in pts] == inf                                      # 1. infinities exactly where the flags say
    if not is_g2:                                                                     # 2. the library's own curve check
        srs = gpu.Srs.from_host(pts)
        rep = srs.check_curve()
        srs.release()
        assert (rep["checked"], rep["infinity"], rep["non_canonical"], rep["off_curve"], rep["first_bad"]) == (len(encs), sum(inf), 0, 0, None)
    back, st2 = (codec.g2_compress if is_g2 else codec.g1_compress)(pts)              # 3. the root was chosen right iff this holds
    assert not st2.any() and back.tobytes() == b"".join(encs)
    full = name in ("beta_g2", "gamma_g2", "delta_g2", "b_g2_query")                  # 4. the restatement, G2 in full
    idx = list(range(len(encs))) if full else _sample(encs)
    got = (g2_points if is_g2 else g1_points)(pts[idx])
    if is_g2:
        assert got == [g2.decompress_g2(encs[i]) for i in idx]
    else:
        assert got == [cr.g1_decompress(encs[i])[1] for i in idx]


def test_register_compressed(gpu, codec, key):
    data, layout = key
    encs = cr.section_encodings(data, layout, "l_query")[:300]
    pts, _ = codec.g1_decompress(b"".join(encs))
    srs = gpu.Srs(codec.srs_register_compressed(b"".join(encs)), len(encs))
    assert np.array_equal(srs.download(), pts) and srs.check_curve()["off_curve"] == 0
    srs.release()
    from uzkge_amd.errors import UzkgeError
    with pytest.raises(UzkgeError, match="point 7"):
        codec.srs_register_compressed(b"".join(encs[:7]) + _g1_bad()["no point"] + b"".join(encs[8:]))
    e2 = cr.section_encodings(data, layout, "b_g2_query")[:70]
    bases = gpu.G2Bases(codec.g2_register_compressed(b"".join(e2), check_subgroup=True), len(e2))
    assert bases.len() == len(e2)
    scal = g2.scalars_to_wire([1] * len(e2))
    want = g2.msm([g2.decompress_g2(e) for e in e2], [1] * len(e2))
    assert g2_points(gpu.g2_to_affine(gpu.msm_g2(bases, scal)).reshape(1, 16)) == [want]
    bases.release()
    with pytest.raises(UzkgeError, match="point 3"):
        codec.g2_register_compressed(b"".join(e2[:3]) + cr.g2_compress(cr.g2_outside_subgroup()) + b"".join(e2[4:]), check_subgroup=True)


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def circuits(gpu, key):
    from uzkge_amd import reveal_cs
    data, _ = key
    old = reveal_cs.RevealCircuit.from_key_bytes(data)                                # the existing path: Python integers, ~4 s
    new = reveal_cs.RevealCircuit.from_compressed(data)
    yield old, new
    old.release()
    new.release()


def test_proofs_of_a_device_decoded_key(gpu, key, circuits):
    from uzkge_amd import poly_commit as pc
    data, _ = key
    old, new = circuits
    assert new.n_vars == old.n_vars == 4869
    sk = _rng.randrange(1, ed.L)
    cards = ed.rand_subgroup_points(3, 11)
    r, s = [_rng.randrange(1, Q) for _ in range(3)], [_rng.randrange(1, Q) for _ in range(3)]
    st_old, proofs_old = old.prove(sk, cards, r, s)
    st_new, proofs_new = new.prove(sk, cards, r, s)
    assert st_new == st_old and proofs_new == proofs_old                              # byte for byte
    vk = pc.Groth16VerifierKey.from_compressed(data[:456])
    vk_old = pc.Groth16VerifierKey.from_key_bytes(data[:456])
    assert vk.n_inputs == vk_old.n_inputs == 7
    for a, b in ((vk.key.beta_g2, vk_old.key.beta_g2), (vk.key.gamma_g2, vk_old.key.gamma_g2), (vk.key.delta_g2, vk_old.key.delta_g2)):
        assert np.array_equal(a, b)
    weights = [_rng.randrange(1, 1 << 128) for _ in range(3)]
    accepted, status = vk.verify_batch(proofs_new, [list(t) for t in st_new], weights)
    assert accepted and not status.any()
    assert vk_old.verify_batch(proofs_new, [list(t) for t in st_new], weights)[0]
    bent = [list(t) for t in st_new]
    bent[1][3] = (bent[1][3] + 1) % Q
    accepted, status = vk.verify_batch(proofs_new, bent, weights)
    assert not accepted and not status.any()
    vk.release()
    vk_old.release()
    whole = pc.Groth16VerifierKey.from_compressed(data, validate=True)                # a proving key's head is a verifying key
    assert whole.verify_batch(proofs_new, [list(t) for t in st_new], weights)[0]
    whole.release()


def test_validated_load(gpu, key):
    from uzkge_amd import reveal_cs
    from uzkge_amd.errors import UzkgeError
    data, layout = key
    off, count = layout["b_g2_query"]
    k = next(i for i in range(count) if not data[off + 64 * i + 63] & 0x40)
    flipped = bytearray(data)
    flipped[off + 64 * k + 63] ^= 0x80                                                # -Q is as good a point as Q
    c = reveal_cs.RevealCircuit.from_compressed(bytes(flipped), validate=True)
    assert c.n_vars == 4869
    c.release()
    bad = bytearray(data)
    bad[off + 64 * 5:off + 64 * 6] = cr.g2_compress(cr.g2_outside_subgroup())
    with pytest.raises(UzkgeError, match=r"b_g2_query\[5\]"):
        reveal_cs.RevealCircuit.from_compressed(bytes(bad), validate=True)
    c = reveal_cs.RevealCircuit.from_compressed(bytes(bad), validate=False)           # on the twist: taken on trust without validate
    c.release()
    bad = bytearray(data)
    a_off = layout["a_query"][0]
    bad[a_off + 32 * 9:a_off + 32 * 10] = _g1_bad()["no point"]
    with pytest.raises(UzkgeError, match=r"a_query\[9\]"):
        reveal_cs.RevealCircuit.from_compressed(bytes(bad))
    with pytest.raises(UzkgeError, match="l_query"):
        reveal_cs.RevealCircuit.from_compressed(data[:-1])


# ---- cards ------------------------------------------------------------------------------------------------------------------------------
def test_cards(gpu):
    from uzkge_amd import reveal as rv
    ys = cr.card_ys()
    pts = rv.points_from_y(ys)
    assert pts == [cr.ed_decompress((y | 1 << 255).to_bytes(32, "little"))[1] for y in ys]
    assert not gpu.ed_check_points(rv.points_to_wire(pts)).any()
    small = rv.points_from_y(ys[:5], greatest=False)
    assert small == [((-p[0]) % Q, p[1]) for p in pts[:5]]
    assert rv.points_from_y([1, Q - 1]) == [(0, 1), (0, Q - 1)]
    deck = ed.rand_subgroup_points(52, 77)
    strings = ["0x" + cr.ed_compress(p).hex() for p in deck]
    assert rv.points_from_hex(strings) == deck and rv.points_to_hex(rv.points_from_hex(strings)) == strings
    assert rv.points_to_hex(deck[:2], with_start=False) == [s[2:] for s in strings[:2]]
    with pytest.raises(ValueError, match="point 1: status 3"):
        rv.points_from_hex([strings[0], cr.ed_compress(ed.order8_point()).hex()])
    assert rv.points_from_hex([cr.ed_compress(ed.order8_point()).hex()], check_subgroup=False) == [ed.order8_point()]
