// The layout of the reveal circuit: the calls RevealCircuit::generate_constraints (shuffle/src/reveal_with_snark.rs) makes on a
// constraint system through ark-r1cs-std 0.4's twisted Edwards gadget, in their order, with no values.  A field variable is a constant
// or a linear combination over the variables (ark-relations inlines its symbolic combinations before it writes the matrices); a
// product of two variables allocates a witness and a row.  Plain C++17: tests/cpp/revealcs_host.cpp builds this file with g++ and
// sanitizers.
#include <map>

#include "revealcs.hpp"
#include "revealcs_consts.inc"

namespace uzk {

namespace {

Fp words(const uint32_t (&w)[8]) { Fp r; for (int i = 0; i < 8; ++i) r.v[i] = w[i]; return r; }

// FpVar: Constant (one term on the variable one, or none) or Var
struct Lc {
    bool is_const = true;
    std::map<uint32_t, Fp> t;
};
struct Pt { Lc x, y; };

Lc constant(const Fp& v) { Lc r; if (!Fr::is_zero(v)) r.t[0] = v; return r; }
Fp const_value(const Lc& a) { auto it = a.t.find(0); return it == a.t.end() ? Fr::zero() : it->second; }

// kx x + ky y
Lc lin(const Lc& x, const Fp& kx, const Lc& y, const Fp& ky) {
    Lc r;
    r.is_const = x.is_const && y.is_const;
    for (const auto& kv : x.t) r.t[kv.first] = Fr::mul(kv.second, kx);
    for (const auto& kv : y.t) {
        auto it = r.t.find(kv.first);
        const Fp v = Fr::mul(kv.second, ky);
        if (it == r.t.end()) r.t[kv.first] = v; else it->second = Fr::add(it->second, v);
    }
    return r;
}

struct Builder {
    RevealLayout& L;
    const Fp one = Fr::one(), minus_one = Fr::neg(Fr::one()), zero = Fr::zero(), two = Fr::add(Fr::one(), Fr::one()), d = words(kRcsD);
    const Lc lc_one = constant(Fr::one()), lc_zero = constant(Fr::zero());
    explicit Builder(RevealLayout& l) : L(l) {
        for (auto& m : L.mat) m.row_ptr.assign(1, 0);
        L.roles.assign(1, kRcsNoRole);
    }
    Lc var(uint32_t role) {
        Lc r;
        r.is_const = false;
        r.t[(uint32_t)L.roles.size()] = one;
        L.roles.push_back(role);
        return r;
    }
    void row(RcsMatrix& m, const Lc& a) {
        for (const auto& kv : a.t)
            if (!Fr::is_zero(kv.second)) { m.col.push_back(kv.first); m.val.push_back(kv.second); }
        m.row_ptr.push_back(m.col.size());
    }
    void enforce(const Lc& a, const Lc& b, const Lc& c) { row(L.mat[0], a); row(L.mat[1], b); row(L.mat[2], c); }
    Lc add(const Lc& x, const Lc& y) { return lin(x, one, y, one); }
    Lc sub(const Lc& x, const Lc& y) { return lin(x, one, y, minus_one); }
    Lc scale(const Lc& x, const Fp& k) { return lin(x, k, lc_zero, zero); }
    Lc addc(const Lc& x, const Fp& k) { return lin(x, one, lc_one, k); }
    // a constant operand scales the other one, which stays a Var even under the factor 0
    Lc mul(const Lc& x, const Lc& y, uint32_t role) {
        if (x.is_const || y.is_const) {
            Lc r = x.is_const ? scale(y, const_value(x)) : scale(x, const_value(y));
            r.is_const = x.is_const && y.is_const;
            return r;
        }
        const Lc w = var(role);
        enforce(x, y, w);
        return w;
    }
    // cond t + (1 - cond) f of two constants is linear; else cond (t - f) = r - f
    Lc select(const Lc& bit, const Lc& t, const Lc& f, uint32_t role) {
        if (t.is_const && f.is_const) return lin(bit, Fr::sub(const_value(t), const_value(f)), lc_one, const_value(f));
        const Lc r = var(role);
        enforce(bit, sub(t, f), sub(r, f));
        return r;
    }
    void enforce_equal(const Lc& x, const Lc& y) { enforce(sub(x, y), lc_one, lc_zero); }

    // an input point: x2 = x x, y2 = y y, (d x2 - 1) y2 = a x2 - 1 with a = 1
    void input_point(const Pt& p, uint32_t k) {
        const Lc x2 = mul(p.x, p.x, rcs_role(kRcsPoint, k, kRcsX2)), y2 = mul(p.y, p.y, rcs_role(kRcsPoint, k, kRcsY2));
        enforce(addc(scale(x2, d), minus_one), y2, addc(x2, minus_one));
    }
    // this + other, both not constant at once: u = (-a x1 + y1)(x2 + y2), v0 = y2 x1, v1 = x2 y1, v2 = d v0 v1,
    // x3 (1 + v2) = v0 + v1, y3 (1 - v2) = u + a v0 - v1
    Pt add_points(const Pt& a, const Pt& b, uint32_t chain, uint32_t it) {
        const Lc u = mul(add(scale(a.x, minus_one), a.y), add(b.x, b.y), rcs_role(chain, it, kRcsU));
        const Lc v0 = mul(b.y, a.x, rcs_role(chain, it, kRcsV0)), v1 = mul(b.x, a.y, rcs_role(chain, it, kRcsV1));
        const Lc v2 = scale(mul(v0, v1, rcs_role(chain, it, kRcsV0V1)), d);
        Pt r;
        r.x = var(rcs_role(chain, it, kRcsX3));
        enforce(r.x, addc(v2, one), add(v0, v1));
        r.y = var(rcs_role(chain, it, kRcsY3));
        enforce(r.y, scale(addc(v2, minus_one), minus_one), sub(add(u, v0), v1));
        return r;
    }
    // xy, x2, y2; x3 (a x2 + y2) = 2 xy, y3 (2 - a x2 - y2) = y2 - a x2
    Pt double_point(const Pt& p, uint32_t chain, uint32_t it) {
        const Lc xy = mul(p.x, p.y, rcs_role(chain, it, kRcsXY)), x2 = mul(p.x, p.x, rcs_role(chain, it, kRcsDX2)), y2 = mul(p.y, p.y, rcs_role(chain, it, kRcsDY2));
        const Lc s = add(x2, y2);
        Pt r;
        r.x = var(rcs_role(chain, it, kRcsDX3));
        enforce(r.x, s, scale(xy, two));
        r.y = var(rcs_role(chain, it, kRcsDY3));
        enforce(r.y, addc(scale(s, minus_one), two), sub(y2, x2));
        return r;
    }
    // scalar_mul_le: res = 0, multiple = base; per bit tmp = res + multiple, res = bit.select(tmp, res), multiple.double_in_place().
    // A constant base doubles through the table of 2^i G; 0 + a constant is that constant.
    Pt scalar_mul(const Pt* base, const std::vector<Lc>& bits, uint32_t chain) {
        Pt res, multiple;
        res.x = lc_zero; res.y = lc_one;
        if (base) multiple = *base;
        for (uint32_t it = 0; it < kRcsBits; ++it) {
            if (!base) { multiple.x = constant(words(kRcsMultiples[it][0])); multiple.y = constant(words(kRcsMultiples[it][1])); }
            const bool all_const = res.x.is_const && res.y.is_const && !base;
            const Pt tmp = all_const ? multiple : add_points(res, multiple, chain, it);
            Pt next;
            next.x = select(bits[it], tmp.x, res.x, rcs_role(chain, it, kRcsSelX));
            next.y = select(bits[it], tmp.y, res.y, rcs_role(chain, it, kRcsSelY));
            res = next;
            if (base) multiple = double_point(multiple, chain, it);
        }
        return res;
    }
};

}  // namespace

bool reveal_layout_build(RevealLayout* out) {
    *out = RevealLayout();
    RevealLayout& L = *out;
    Builder B(L);
    Pt pts[3];                                                     // h, reveal, pk
    for (Pt& p : pts) { p.x = B.var(kRcsNoRole); p.y = B.var(kRcsNoRole); }
    for (uint32_t k = 0; k < 3; ++k) B.input_point(pts[k], k);
    std::vector<Lc> bits;
    for (uint32_t i = 0; i < kRcsBits; ++i) {
        const Lc b = B.var(rcs_role(kRcsBit, i, kRcsBitRole));
        B.enforce(lin(B.lc_one, B.one, b, B.minus_one), b, B.lc_zero);             // (1 - b) b = 0
        bits.push_back(b);
    }
    const Pt t1 = B.scalar_mul(nullptr, bits, kRcsFixed);
    B.enforce_equal(t1.x, pts[2].x); B.enforce_equal(t1.y, pts[2].y);
    const Pt t2 = B.scalar_mul(&pts[0], bits, kRcsVar);
    B.enforce_equal(t2.x, pts[1].x); B.enforce_equal(t2.y, pts[1].y);
    L.n_vars = (uint32_t)L.roles.size(); L.n_inputs = kRcsInputs; L.n_constraints = (uint32_t)L.mat[0].row_ptr.size() - 1;
    L.domain = 1;
    while (L.domain < (uint64_t)L.n_constraints + L.n_inputs) L.domain <<= 1;
    for (uint32_t i = 0; i < kRcsBits; ++i)
        for (int c = 0; c < 2; ++c) L.multiples.push_back(words(kRcsMultiples[i][c]));
    return L.n_vars == kRcsVars && L.n_constraints == kRcsConstraints && L.domain == kRcsDomain;
}

}  // namespace uzk
