// Baby Jubjub on the device: the arithmetic a reveal is made of, batched one lane per item (ed29.hpp has the group law).
//
//   ed_check        one lane per point: canonical words, the curve equation, [L] P = identity (the bits of L are the same for every lane)
//   ed_mul          one lane per item: s_i P_i over the 256 bits of s_i by double-and-add with the unified addition, then the affine map
//                   with the inversion in the lane; a point stride of 0 shares one base
//   ed_sum          one lane per card j: sum_k P_kj over k rows of n points, or e2_j - sum_k P_kj (unmask)
//   cp_transcript   one lane per DL proof over the parameters (g, h) and the statement (u, v): Keccak-256 of the 448-byte transcript
//                   label | "DL" | g, h, u, v, a, b; c = digest mod L; for a prover also r = omega + c secret mod L and the proof blob.
//                   A reveal is (e1, G; reveal, pk) under "Revealing", a mask (G, pk; e1, e2 - card) under "Masking".  The zk-friendly
//                   reveal (dl.rs prove0 / verify0) is the same lane in its second transcript mode: c = the Anemoi-Jive hash of the
//                   twelve coordinates (anemoi29.hpp, four permutations), taken as an integer below r, mod L
//   cp_mask_diff    one lane per mask proof: e2 - card in affine, the second point of its statement
//   cp_check        ONE launch for the two chains of a verification, each kind of lane in workgroups of its own:
//                     one lane per point (a reveal: e1, reveal, pk; a mask: pk, card, e1, e2; then a and b from the 160-byte blob):
//                     decode, then ed_check's classification;
//                     one lane per equation, two per proof: r P - c Q by Straus / Shamir over the joint bits of (r, c) with the table
//                     {P, -Q, P - Q} in ONE doubling chain, compared projectively with a (or b):  r g = a + c u,  r h = b + c v
//   cp_verdict      one lane per proof: the first failing check as the verdict byte
//   cp_prove_mul    one lane per multiplication of a batch of proofs: 3 m + 1 for reveals (sk e1_i, omega_i e1_i, omega_i G and sk G),
//                   5 m for masks (r_i G, card_i + r_i pk, omega_i G, omega_i pk, r_i pk)
//   remark_table    one launch per table, lane i = segment i of T_P[i][j] = (j + 1) 16^i P: 4 i doublings, three additions, one inversion
//   remark          one lane per (card, component) of a shuffle's remask: 84 additions of the table entry the digit names; with a trace,
//                   every step's affine point from ONE inversion per lane (Montgomery's trick along the chain, through a workspace)
//
// Every chain is 256 unified additions-with-doubling long whatever the batch: the latency of a call is the chain, not the lane count
// (52 proofs are 104 lanes, two waves); a remask's is 84 additions.  tests/ed_ref.py and tests/shuffle_ref.py are the restatements on
// Python integers.
#include <cstring>

#include "anemoi29.hpp"
#include "ctx.hpp"
#include "ed29.hpp"
#include "handles.hpp"
#include "lane_tools.hpp"

namespace uzk {

constexpr uint32_t kEdBlock = 64;
static_assert(sizeof(EdAffine) == 64, "a point is eight 64-bit words on the wire");
static_assert(UZK_CP_PROOF_BYTES == 160, "a proof is five 32-byte words");

// a blob is 32-byte big-endian words (load_be32 / store_be32 of lane_tools.hpp); blobs are 160 bytes apart in a 256-byte aligned array

__global__ __launch_bounds__(kEdBlock) void ed_check_kernel(const EdAffine* __restrict__ pts, uint8_t* __restrict__ status, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kEdBlock + threadIdx.x;
    if (i >= n) return;
    status[i] = (uint8_t)ed::classify(pts[i]);
#endif
}

__global__ __launch_bounds__(kEdBlock) void ed_mul_kernel(const EdAffine* __restrict__ pts, uint32_t point_stride, const Fp* __restrict__ scalars,
                                                           EdAffine* __restrict__ out, uint32_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kEdBlock + threadIdx.x;
    if (i >= n) return;
    out[i] = ed::to_affine(ed::mul(ed::from_affine(pts[(size_t)i * point_stride]), scalars[i]));
#endif
}

// out_j = sum_k rows[k n + j], or e2_j minus that sum
__global__ __launch_bounds__(kEdBlock) void ed_sum_kernel(const EdAffine* __restrict__ rows, uint32_t k, uint32_t n, const EdAffine* __restrict__ e2,
                                                           EdAffine* __restrict__ out) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t j = blockIdx.x * kEdBlock + threadIdx.x;
    if (j >= n) return;
    ed::P acc = ed::identity();
#pragma unroll 1
    for (uint32_t r = 0; r < k; ++r) acc = ed::add(acc, ed::from_affine(rows[(size_t)r * n + j]));
    if (e2) acc = ed::add(ed::from_affine(e2[j]), ed::neg(acc));
    out[j] = ed::to_affine(acc);
#endif
}

// The DL proof i over the parameters (g, h) and the statement (u, v):  r g = a + c u,  r h = b + c v.  Each point comes through its own
// pointer and stride (a verifier's buffer holds a statement's points side by side, a prover has them in arrays of their own, a stride of
// 0 shares one point); a null pointer is the generator.
//   a reveal   g = e1, h = G, u = reveal, v = pk            under "Revealing"; classified: e1, reveal, pk
//   a mask     g = G,  h = pk, u = e1,    v = e2 - card     under "Masking";   classified: pk, card, e1, e2
// cls: the n_cls points of the statement that go through ed::classify beside a and b of the blob.
struct CpStatement {
    const EdAffine *g, *h, *u, *v;
    uint32_t s_g, s_h, s_u, s_v;
    const EdAffine *c0, *c1, *c2, *c3;
    uint32_t s_c0, s_c1, s_c2, s_c3;
    uint32_t n_cls;
    CpLabel label;
    uint32_t transcript;               // kCpKeccak: Keccak-256 under `label`; kCpAnemoi: the Anemoi-Jive hash of the twelve coordinates
};
constexpr uint32_t kCpKeccak = 0, kCpAnemoi = 1;
__device__ __forceinline__ EdAffine cp_at(const EdAffine* p, uint32_t stride, uint32_t i) { return p ? p[(size_t)i * stride] : ed_generator(); }

// a (which = 0) or b (which = 1) of a blob in Montgomery words; false (and zeros) when a word is not below q
__device__ __forceinline__ bool cp_blob_point(const uint8_t* blob, uint32_t which, EdAffine* p) {
    const Fp x = load_be32(blob + 64 * which), y = load_be32(blob + 64 * which + 32);
    const bool canonical = ed_coord_canonical(x) && ed_coord_canonical(y);
    p->x = canonical ? Fr::to_mont(x) : Fr::zero();
    p->y = canonical ? Fr::to_mont(y) : Fr::zero();
    return canonical;
}

// Coordinate k (g.x g.y h.x h.y u.x u.y v.x v.y a.x a.y b.x b.y) of proof i as the Anemoi transcript takes it: canonical Montgomery
// words, the identity as anemoi_cp_point_words encodes it.  A point with a word not below q -- a verifier's statement and blob are
// not checked before this lane runs -- enters as zeros: the limbs' contract holds, and the point lanes of cp_check give that proof
// verdict 1 whatever its challenge is.
__device__ __forceinline__ Fp cp_anemoi_word(const CpStatement& s, const uint8_t* proofs_in, const EdAffine* ab, uint32_t i, uint32_t k) {
    const uint32_t pt = k >> 1;
    EdAffine p;
    if (pt < 4) p = pt == 0 ? cp_at(s.g, s.s_g, i) : pt == 1 ? cp_at(s.h, s.s_h, i) : pt == 2 ? cp_at(s.u, s.s_u, i) : cp_at(s.v, s.s_v, i);
    else if (proofs_in) (void)cp_blob_point(proofs_in + (size_t)i * UZK_CP_PROOF_BYTES, pt - 4, &p);
    else p = ab[2 * (size_t)i + (pt - 4)];
    if (!ed_coord_canonical(p.x) || !ed_coord_canonical(p.y)) { p.x = Fr::zero(); p.y = Fr::zero(); }
    Fp x, y;
    anemoi_cp_point_words(p.x, p.y, &x, &y);
    return (k & 1) ? y : x;
}

// c_i (plain words, below L) from the statement and a, b -- read from the blobs (a verifier: plain big-endian words as they are) or,
// with proofs_in == nullptr, from ab (a prover: Montgomery words of the points it has just computed); with omega also
// r_i = omega_i + c_i sk_i mod L (sk_i = sk[i s_sk]: one secret for a player's reveals, one r per masked card) and the blob
// a.x a.y b.x b.y r
__global__ __launch_bounds__(kEdBlock) void cp_transcript_kernel(CpStatement s, const uint8_t* __restrict__ proofs_in, const EdAffine* __restrict__ ab,
                                                                  Fp* __restrict__ c_out, const Fp* __restrict__ omega, const Fp* __restrict__ sk, uint32_t s_sk,
                                                                  uint8_t* __restrict__ proofs_out, uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kEdBlock + threadIdx.x;
    if (i >= m) return;
    const EdAffine pts[4] = {cp_at(s.g, s.s_g, i), cp_at(s.h, s.s_h, i), cp_at(s.u, s.s_u, i), cp_at(s.v, s.s_v, i)};
    Fp w[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) { w[2 * k] = Fr::from_mont(pts[k].x); w[2 * k + 1] = Fr::from_mont(pts[k].y); }
    if (proofs_in) {
#pragma unroll
        for (int k = 0; k < 4; ++k) w[8 + k] = load_be32(proofs_in + (size_t)i * UZK_CP_PROOF_BYTES + 32 * k);
    } else {
#pragma unroll
        for (int k = 0; k < 2; ++k) { w[8 + 2 * k] = Fr::from_mont(ab[2 * (size_t)i + k].x); w[9 + 2 * k] = Fr::from_mont(ab[2 * (size_t)i + k].y); }
    }
    Fp digest;
    if (s.transcript == kCpAnemoi) {
        Fp h;
        anemoi::sponge([&](uint32_t k) { return cp_anemoi_word(s, proofs_in, ab, i, k); }, 12, 0, &h, nullptr);
        digest = Fr::from_mont(h);                                 // an integer below r: floor(r / L) = 7
    } else {
        digest = cp_transcript_digest(w, s.label);
    }
    const Fp c = ed_mod_order(digest);
    c_out[i] = c;
    if (omega) {
        const Fp r = ed_muladd_order(ed_mod_order(omega[i]), c, ed_mod_order(sk[(size_t)i * s_sk]));
        uint8_t* blob = proofs_out + (size_t)i * UZK_CP_PROOF_BYTES;
#pragma unroll
        for (int k = 0; k < 4; ++k) store_be32(blob + 32 * k, w[8 + k]);
        store_be32(blob + 128, r);
    }
#endif
}

// v_i = e2_i - card_i of a mask in affine, what its transcript and its second equation are about; zeros where a coordinate is not
// below q (the point lanes of cp_check report that proof with verdict 1)
__global__ __launch_bounds__(kEdBlock) void cp_mask_diff_kernel(const EdAffine* __restrict__ e2, const EdAffine* __restrict__ cards, EdAffine* __restrict__ diff,
                                                                 uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kEdBlock + threadIdx.x;
    if (i >= m) return;
    const EdAffine a = e2[i], b = cards[i];
    EdAffine r;
    r.x = Fr::zero(); r.y = Fr::zero();
    if (ed_coord_canonical(a.x) && ed_coord_canonical(a.y) && ed_coord_canonical(b.x) && ed_coord_canonical(b.y))
        r = ed::to_affine(ed::add(ed::from_affine(a), ed::neg(ed::from_affine(b))));
    diff[i] = r;
#endif
}

// The two chains of a verification in ONE launch, each kind of lane in workgroups of its own (a wave runs one control flow), with
// np = s.n_cls + 2 points per proof:
//   workgroups [0, point_blocks)   lane np i + w: point w of proof i -- the statement's classified points, then a and b from the blob --
//                                  through ed_check's classification into pst[np i + w]
//   the workgroups behind them     lane 2 i + q: equation q of proof i into ok[2 i + q]:  r P - c Q = a (b) with P = g (h), Q = u (v)
// The equation lanes do not wait for the points' verdicts: they refuse only what would break the limbs' contract (a word not below q)
// and compute on whatever else they are given -- cp_verdict reads an equation only where all points passed.
__global__ __launch_bounds__(kEdBlock) void cp_check_kernel(CpStatement s, const uint8_t* __restrict__ proofs, const Fp* __restrict__ c,
                                                             uint8_t* __restrict__ pst, uint8_t* __restrict__ ok, uint32_t m, uint32_t point_blocks) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (blockIdx.x < point_blocks) {
        const uint32_t np = s.n_cls + 2;
        const uint32_t t = blockIdx.x * kEdBlock + threadIdx.x;
        if (t >= np * m) return;
        const uint32_t i = t / np, w = t % np;
        EdAffine p;
        uint32_t st = 0;
        if (w >= s.n_cls) st = cp_blob_point(proofs + (size_t)i * UZK_CP_PROOF_BYTES, w - s.n_cls, &p) ? 0 : 1;
        else p = w == 0 ? cp_at(s.c0, s.s_c0, i) : w == 1 ? cp_at(s.c1, s.s_c1, i) : w == 2 ? cp_at(s.c2, s.s_c2, i) : cp_at(s.c3, s.s_c3, i);
        if (st == 0) st = ed::classify(p);
        pst[t] = (uint8_t)st;
        return;
    }
    const uint32_t t = (blockIdx.x - point_blocks) * kEdBlock + threadIdx.x;
    if (t >= 2 * m) return;
    const uint32_t i = t >> 1, q = t & 1;
    const uint8_t* blob = proofs + (size_t)i * UZK_CP_PROOF_BYTES;
    const EdAffine base = q == 0 ? cp_at(s.g, s.s_g, i) : cp_at(s.h, s.s_h, i);
    const EdAffine other = q == 0 ? cp_at(s.u, s.s_u, i) : cp_at(s.v, s.s_v, i);
    EdAffine rhs;
    const bool canonical = cp_blob_point(blob, q, &rhs) && ed_coord_canonical(base.x) && ed_coord_canonical(base.y) && ed_coord_canonical(other.x) &&
                           ed_coord_canonical(other.y);
    if (!canonical) { ok[t] = 0; return; }
    const Fp r = load_be32(blob + 128);                             // any 256-bit integer: an integer multiple is defined on the whole curve
    const ed::P t1 = ed::from_affine(base), t2 = ed::neg(ed::from_affine(other)), t3 = ed::add(t1, t2);
    const ed::P lhs = ed::mul2(t1, t2, t3, r, c[i]);
    ok[t] = ed::eq_affine(lhs, ed::ld(rhs.x), ed::ld(rhs.y)) ? 1 : 0;
#endif
}

// 1 .. 3: the smallest nonzero status among the proof's np points (the codes are in the order of the checks); then 4, 5: the equations
__global__ __launch_bounds__(kEdBlock) void cp_verdict_kernel(const uint8_t* __restrict__ pst, const uint8_t* __restrict__ ok, uint8_t* __restrict__ verdict, uint32_t m,
                                                               uint32_t np) {
    const uint32_t i = blockIdx.x * kEdBlock + threadIdx.x;
    if (i >= m) return;
    uint32_t v = 0;
    for (uint32_t k = 0; k < np; ++k) {
        const uint32_t st = pst[np * (size_t)i + k];
        if (st && (v == 0 || st < v)) v = st;
    }
    if (v == 0) v = !ok[2 * (size_t)i] ? 4 : !ok[2 * (size_t)i + 1] ? 5 : 0;
    verdict[i] = (uint8_t)v;
}

// The multiplications of a batch of proofs, one lane each.
//   reveals (mask == 0), 3 m + 1 lanes   lane 3 i + w: 0 reveal_i = sk e1_i, 1 a_i = omega_i e1_i, 2 b_i = omega_i G; lane 3 m: pk = sk G
//   masks   (mask == 1), 5 m lanes       lane 5 i + w: 0 e1_i = r_i G, 1 e2_i = card_i + r_i pk, 2 a_i = omega_i G, 3 b_i = omega_i pk,
//                                        4 v_i = r_i pk (e2_i - card_i, the statement's second point, without a subtraction)
struct CpProveArgs {
    uint32_t mask;
    const EdAffine* bases;             // reveals: e1; masks: the cards
    const Fp* secret;                  // reveals: sk (one); masks: r (m)
    const Fp* omega;
    const EdAffine* pk_in;             // masks: the joint key
    EdAffine *out0, *out1;             // reveals: reveal, -; masks: e1, e2
    EdAffine* ab;
    EdAffine* extra;                   // reveals: pk = sk G (one); masks: v (m)
};
__global__ __launch_bounds__(kEdBlock) void cp_prove_mul_kernel(CpProveArgs a, uint32_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t t = blockIdx.x * kEdBlock + threadIdx.x;
    const bool mask = a.mask != 0;
    if (t >= (mask ? 5 * m : 3 * m + 1)) return;
    const uint32_t per = mask ? 5 : 3, i = t / per, w = t % per;    // a reveal's t == 3 m: i = m, w = 0 -- no array is read at i then
    const bool is_pk = !mask && t == 3 * m;
    const bool use_gen = mask ? (w == 0 || w == 2) : (is_pk || w == 2);
    const bool use_omega = mask ? (w == 2 || w == 3) : !(is_pk || w == 0);
    const EdAffine* bp = mask ? a.pk_in : a.bases + i;
    const EdAffine base = use_gen ? ed_generator() : *bp;
    const Fp k = *(use_omega ? a.omega + i : mask ? a.secret + i : a.secret);
    ed::P acc = ed::mul(ed::from_affine(base), k);
    if (mask && w == 1) acc = ed::add(acc, ed::from_affine(a.bases[i]));
    EdAffine* dst = mask ? (w == 0 ? a.out0 + i : w == 1 ? a.out1 + i : w == 4 ? a.extra + i : a.ab + 2 * (size_t)i + (w - 2))
                         : (is_pk ? a.extra : w == 0 ? a.out0 + i : a.ab + 2 * (size_t)i + (w - 1));
    *dst = ed::to_affine(acc);
#endif
}

// ---- the remask of a shuffle (uzkge/src/shuffle/remark.rs) ---------------------------------------------------------------------------
// T_P[i][j] = (j + 1) 16^i P for i < 84, j < 4, each entry the three wire elements x, y, d x y of the affine point.
constexpr uint32_t kRemarkIters = UZK_REMARK_ITERATIONS, kRemarkEntries = kRemarkIters * 4, kRemarkEntryWords = 3;
constexpr size_t kRemarkTableBytes = (size_t)kRemarkEntries * kRemarkEntryWords * sizeof(Fp);

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ void remark_put_entry(Fp* e, const ed::P& p, const ed::C& zi) {
    const ed::C x = ed::Z::mul(p.x, zi), y = ed::Z::mul(p.y, zi);
    e[0] = ed::Z::to_wire(x); e[1] = ed::Z::to_wire(y);
    e[2] = ed::Z::to_wire(ed::Z::mul(ed::Z::mul(x, y), ed::Z::ld(ed_d_wire())));
}
#endif

// One launch per table, lane i = segment i: 16^i P by 4 i doublings, the segment P, 2 P, 3 P, 4 P by three additions, then the affine
// map of the four with ONE inversion (Montgomery's trick over the four Z) and d x y.  No lane waits for another: the latency is the
// longest lane's 332 doublings, the chain a single lane would walk; a null base is the generator.  The unified law makes the
// definition hold on the whole curve (a point of order 8 collapses to the identity after its first doublings).
__global__ __launch_bounds__(kEdBlock) void remark_table_kernel(const EdAffine* __restrict__ base, Fp* __restrict__ table) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t i = blockIdx.x * kEdBlock + threadIdx.x;
    if (i >= kRemarkIters) return;
    ed::P p1 = ed::from_affine(base ? *base : ed_generator());
#pragma unroll 1
    for (uint32_t k = 0; k < 4 * i; ++k) p1 = ed::add(p1, p1);
    const ed::P p2 = ed::add(p1, p1), p3 = ed::add(p2, p1), p4 = ed::add(p3, p1);
    const ed::C z12 = ed::Z::mul(p1.z, p2.z), z34 = ed::Z::mul(p3.z, p4.z);
    const ed::C inv = ed::inv(ed::Z::mul(z12, z34));
    const ed::C i12 = ed::Z::mul(inv, z34), i34 = ed::Z::mul(inv, z12);
    Fp* e = table + (size_t)i * 4 * kRemarkEntryWords;
    remark_put_entry(e, p1, ed::Z::mul(i12, p2.z));
    remark_put_entry(e + 3, p2, ed::Z::mul(i12, p1.z));
    remark_put_entry(e + 6, p3, ed::Z::mul(i34, p4.z));
    remark_put_entry(e + 9, p4, ed::Z::mul(i34, p3.z));
#endif
}

// The remask of `count` cards from card `first` on, one lane per (card, component): lane 2 k + 0 walks c1 = e1_k over T_G, lane 2 k + 1
// walks c2 = e2_k over T_pk, 84 unified additions of the entry its digit names (bit 2 clear: the negated entry (-x, y), T negated with it).
// Without a trace the lane ends with one inversion.  With one, every step's (X, Y, Z) and the prefix product of the Z so far go to the
// lane's column of the workspace ws[step][slot][limb][lane] (consecutive lanes, consecutive words); ONE inversion of the last prefix and
// a walk back along the chain (Montgomery's trick) give the 84 affine points -- 3 products per step instead of an inversion's 380.
// The trace lives at trace[(k - first) 84 + i][c2.x, c2.y, c1.x, c1.y]; entry 83 is also the remasked card, written at the card's output slot.
struct RemarkArgs {
    const Fp *t_gen, *t_pk;
    const EdAffine *e1, *e2;
    const uint8_t* digits;
    const uint32_t* slot;              // the output position of card k (the inverse of perm); null: k
    EdAffine *e1_out, *e2_out;
    Fp* trace;                         // null: no trace
    uint32_t* ws;
    uint32_t first, count;
};
__global__ __launch_bounds__(kEdBlock) void remark_kernel(RemarkArgs a) {
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t t = blockIdx.x * kEdBlock + threadIdx.x, lanes = 2 * a.count;
    if (t >= lanes) return;
    const uint32_t card = a.first + (t >> 1), comp = t & 1;
    const Fp* tab = comp ? a.t_pk : a.t_gen;
    const uint8_t* dg = a.digits + (size_t)card * kRemarkIters;
    EdAffine* out = (comp ? a.e2_out : a.e1_out) + (a.slot ? a.slot[card] : card);
    ed::P acc = ed::from_affine(comp ? a.e2[card] : a.e1[card]);
    ed::C pre = ed::one();
#pragma unroll 1
    for (uint32_t i = 0; i < kRemarkIters; ++i) {
        const uint32_t d = dg[i];
        const Fp* e = tab + ((size_t)i * 4 + (d & 3)) * kRemarkEntryWords;
        EdAffine q;
        q.x = e[0]; q.y = e[1];
        ed::P qp = ed::from_affine(q);
        if (!(d & 4)) qp = ed::neg(qp);
        acc = ed::add(acc, qp);
        if (a.trace) {
            pre = ed::Z::mul(pre, acc.z);
            uint32_t* w = a.ws + (size_t)i * 36 * lanes + t;
#pragma unroll
            for (int l = 0; l < 9; ++l) {
                w[(size_t)l * lanes] = acc.x.v.l[l];
                w[(size_t)(9 + l) * lanes] = acc.y.v.l[l];
                w[(size_t)(18 + l) * lanes] = acc.z.v.l[l];
                w[(size_t)(27 + l) * lanes] = pre.v.l[l];
            }
        }
    }
    if (!a.trace) { *out = ed::to_affine(acc); return; }
    ed::C inv = ed::inv(pre);                                      // 1 / (Z_0 ... Z_83)
    Fp* tr = a.trace + (size_t)(t >> 1) * kRemarkIters * 4 + (comp ? 0 : 2);
#pragma unroll 1
    for (int i = (int)kRemarkIters - 1; i >= 0; --i) {
        const uint32_t* w = a.ws + (size_t)i * 36 * lanes + t;
        ed::C x, y, z, before = ed::one();
#pragma unroll
        for (int l = 0; l < 9; ++l) {
            x.v.l[l] = w[(size_t)l * lanes];
            y.v.l[l] = w[(size_t)(9 + l) * lanes];
            z.v.l[l] = w[(size_t)(18 + l) * lanes];
            if (i > 0) before.v.l[l] = (w - (size_t)36 * lanes)[(size_t)(27 + l) * lanes];
        }
        const ed::C zi = ed::Z::mul(inv, before);                  // 1 / Z_i
        inv = ed::Z::mul(inv, z);                                  // 1 / (Z_0 ... Z_{i-1})
        EdAffine r;
        r.x = ed::Z::to_wire(ed::Z::mul(x, zi)); r.y = ed::Z::to_wire(ed::Z::mul(y, zi));
        tr[(size_t)i * 4] = r.x; tr[(size_t)i * 4 + 1] = r.y;
        if (i == (int)kRemarkIters - 1) *out = r;
    }
#endif
}

// The group law on RAW limbs (uzk_test_ed_raw_kat): coordinates are taken exactly as given -- nothing is re-limbed or reduced on the way
// in, nothing canonicalised on the way out -- so a test can put every coordinate at the edge of ed::C's bound.
struct EdRawPt {
    uint32_t c[4][9];                  // x, y, z, t, nine limbs each (op 5 out: eight wire words of x and y, the ninth 0)
};
struct EdRawIn {
    EdRawPt a, b;
};
struct EdRawOut {
    EdRawPt p;
    uint32_t flag;
};

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ ed::C edraw_c(const uint32_t (&c)[9]) {
    ed::C r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.v.l[i] = c[i];
    return r;
}
__device__ __forceinline__ void edraw_put(uint32_t (&c)[9], const ed::C& x) {
#pragma unroll
    for (int i = 0; i < 9; ++i) c[i] = x.v.l[i];
}
__device__ __forceinline__ void edraw_put_wire(uint32_t (&c)[9], const Fp& w) {
#pragma unroll
    for (int i = 0; i < 8; ++i) c[i] = w.v[i];
    c[8] = 0;
}
__device__ __forceinline__ ed::P edraw_point(const EdRawPt& r) {
    ed::P p;
    p.x = edraw_c(r.c[0]); p.y = edraw_c(r.c[1]); p.z = edraw_c(r.c[2]); p.t = edraw_c(r.c[3]);
    return p;
}
__device__ __forceinline__ void edraw_put_point(EdRawPt& r, const ed::P& p) {
    edraw_put(r.c[0], p.x); edraw_put(r.c[1], p.y); edraw_put(r.c[2], p.z); edraw_put(r.c[3], p.t);
}
#endif

// op 0 add(a, b), 1 neg(a), 2 is_identity(a), 3 eq_affine(a, b.x, b.y), 4 on_curve(a.x, a.y) (the answers in out.flag), 5 to_affine(a) as
// wire words, 6 inv(a.x)
__global__ __launch_bounds__(kEdBlock) void ed_raw_kat_kernel(int op, const EdRawIn* __restrict__ in, EdRawOut* __restrict__ out, size_t n) {
#if defined(__HIP_DEVICE_COMPILE__)
    const size_t i = (size_t)blockIdx.x * kEdBlock + threadIdx.x;
    if (i >= n) return;
    const EdRawIn rec = in[i];
    EdRawOut r;
    for (int k = 0; k < 4; ++k)
        for (int l = 0; l < 9; ++l) r.p.c[k][l] = 0;
    r.flag = 0;
    const ed::P a = edraw_point(rec.a);
    if (op == 0) edraw_put_point(r.p, ed::add(a, edraw_point(rec.b)));
    else if (op == 1) edraw_put_point(r.p, ed::neg(a));
    else if (op == 2) r.flag = ed::is_identity(a);
    else if (op == 3) r.flag = ed::eq_affine(a, edraw_c(rec.b.c[0]), edraw_c(rec.b.c[1]));
    else if (op == 4) r.flag = ed::on_curve(a.x, a.y);
    else if (op == 5) {
        const EdAffine w = ed::to_affine(a);
        edraw_put_wire(r.p.c[0], w.x); edraw_put_wire(r.p.c[1], w.y);
    } else {
        edraw_put(r.p.c[0], ed::inv(a.x));
    }
    out[i] = r;
#endif
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
static unsigned ed_grid(size_t lanes) { return (unsigned)((lanes + kEdBlock - 1) / kEdBlock); }

// the first coordinate of `count` wire elements that is not below q, or count
size_t ed_first_noncanonical(const Fp* words, size_t count) {
    for (size_t i = 0; i < count; ++i)
        if (!ed_coord_canonical(words[i])) return i;
    return count;
}

int ed_check_run(Ctx& c, const EdAffine* pts, size_t n, uint8_t* status_out) {
    WsCarver cv;
    const auto a_pts = cv.array<EdAffine>(n);
    const auto a_st = cv.array<uint8_t>(n);
    UZK_TRY(cv.reserve(c.ed_ws));
    EdAffine* d_pts = cv(a_pts);
    uint8_t* d_st = cv(a_st);
    UZK_HIP(hipMemcpyAsync(d_pts, pts, n * sizeof(EdAffine), hipMemcpyHostToDevice, c.stream));
    UZK_LAUNCH(c, "ed_check", ed_check_kernel, dim3(ed_grid(n)), dim3(kEdBlock), 0, c.stream, d_pts, d_st, (uint32_t)n);
    UZK_HIP(hipMemcpyAsync(status_out, d_st, n, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

int ed_mul_run(Ctx& c, const EdAffine* pts, bool shared_base, const Fp* scalars, size_t n, EdAffine* out) {
    const size_t n_pts = shared_base ? 1 : n;
    WsCarver cv;
    const auto a_pts = cv.array<EdAffine>(n_pts);
    const auto a_sc = cv.array<Fp>(n);
    const auto a_out = cv.array<EdAffine>(n);
    UZK_TRY(cv.reserve(c.ed_ws));
    EdAffine *d_pts = cv(a_pts), *d_out = cv(a_out);
    Fp* d_sc = cv(a_sc);
    UZK_HIP(hipMemcpyAsync(d_pts, pts, n_pts * sizeof(EdAffine), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_sc, scalars, n * sizeof(Fp), hipMemcpyHostToDevice, c.stream));
    UZK_LAUNCH(c, "ed_mul", ed_mul_kernel, dim3(ed_grid(n)), dim3(kEdBlock), 0, c.stream, d_pts, shared_base ? 0u : 1u, d_sc, d_out, (uint32_t)n);
    UZK_HIP(hipMemcpyAsync(out, d_out, n * sizeof(EdAffine), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

// e2 == nullptr: the plain sum
int ed_sum_run(Ctx& c, const EdAffine* e2, const EdAffine* rows, uint32_t k, uint32_t n, EdAffine* out) {
    const size_t row_bytes = (size_t)k * n * sizeof(EdAffine), n_bytes = (size_t)n * sizeof(EdAffine);
    WsCarver cv;
    const auto a_rows = cv.array<EdAffine>((size_t)k * n), a_e2 = cv.array<EdAffine>(n), a_out = cv.array<EdAffine>(n);
    UZK_TRY(cv.reserve(c.ed_ws));
    EdAffine *d_rows = cv(a_rows), *d_e2 = cv(a_e2), *d_out = cv(a_out);
    UZK_HIP(hipMemcpyAsync(d_rows, rows, row_bytes, hipMemcpyHostToDevice, c.stream));
    if (e2) UZK_HIP(hipMemcpyAsync(d_e2, e2, n_bytes, hipMemcpyHostToDevice, c.stream));
    UZK_LAUNCH(c, e2 ? "ed_unmask" : "ed_sum", ed_sum_kernel, dim3(ed_grid(n)), dim3(kEdBlock), 0, c.stream, d_rows, k, n, e2 ? d_e2 : nullptr, d_out);
    UZK_HIP(hipMemcpyAsync(out, d_out, n_bytes, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

// the three kernels of a verification over the statement s (device pointers), and the results to the host
static int cp_verify_launch(Ctx& c, const CpStatement& s, const uint8_t* d_proofs, Fp* d_c, uint8_t* d_pst, uint8_t* d_ok, uint8_t* d_verdict, uint32_t m,
                            uint8_t* verdict_out, Fp* challenges_out) {
    const uint32_t np = s.n_cls + 2;
    UZK_LAUNCH(c, "cp_transcript", cp_transcript_kernel, dim3(ed_grid(m)), dim3(kEdBlock), 0, c.stream, s, d_proofs, nullptr, d_c, nullptr, nullptr, 0u, nullptr, m);
    const unsigned point_blocks = ed_grid((size_t)m * np);
    UZK_LAUNCH(c, "cp_check", cp_check_kernel, dim3(point_blocks + ed_grid((size_t)m * 2)), dim3(kEdBlock), 0, c.stream, s, d_proofs, d_c, d_pst, d_ok, m, point_blocks);
    UZK_LAUNCH(c, "cp_verdict", cp_verdict_kernel, dim3(ed_grid(m)), dim3(kEdBlock), 0, c.stream, d_pst, d_ok, d_verdict, m, np);
    UZK_HIP(hipMemcpyAsync(verdict_out, d_verdict, m, hipMemcpyDeviceToHost, c.stream));
    if (challenges_out) UZK_HIP(hipMemcpyAsync(challenges_out, d_c, (size_t)m * sizeof(Fp), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

// statements: m x (e1, reveal, pk); proofs: m blobs; challenges_out optional (m x plain words); anemoi: the zk-friendly transcript
int cp_verify_run(Ctx& c, const EdAffine* statements, const uint8_t* proofs, uint32_t m, uint8_t* verdict_out, Fp* challenges_out, bool anemoi) {
    WsCarver cv;
    const auto a_stmt = cv.array<EdAffine>((size_t)m * 3);
    const auto a_proofs = cv.array<uint8_t>((size_t)m * UZK_CP_PROOF_BYTES);
    const auto a_c = cv.array<Fp>(m);
    const auto a_pst = cv.array<uint8_t>((size_t)m * 5), a_ok = cv.array<uint8_t>((size_t)m * 2), a_verdict = cv.array<uint8_t>(m);
    UZK_TRY(cv.reserve(c.ed_ws));
    EdAffine* d_stmt = cv(a_stmt);
    uint8_t* d_proofs = cv(a_proofs);
    UZK_HIP(hipMemcpyAsync(d_stmt, statements, (size_t)m * 3 * sizeof(EdAffine), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_proofs, proofs, (size_t)m * UZK_CP_PROOF_BYTES, hipMemcpyHostToDevice, c.stream));
    CpStatement s = {};
    s.g = d_stmt; s.h = nullptr; s.u = d_stmt + 1; s.v = d_stmt + 2;
    s.s_g = s.s_u = s.s_v = 3;
    s.c0 = s.g; s.c1 = s.u; s.c2 = s.v;
    s.s_c0 = s.s_c1 = s.s_c2 = 3;
    s.n_cls = 3;
    s.label = cp_label_revealing();
    s.transcript = anemoi ? kCpAnemoi : kCpKeccak;
    return cp_verify_launch(c, s, d_proofs, cv(a_c), cv(a_pst), cv(a_ok), cv(a_verdict), m, verdict_out, challenges_out);
}

// pk: one point; cards, e1, e2: m points each; proofs: m blobs
int cp_mask_verify_run(Ctx& c, const EdAffine* pk, const EdAffine* cards, const EdAffine* e1, const EdAffine* e2, const uint8_t* proofs, uint32_t m,
                       uint8_t* verdict_out, Fp* challenges_out) {
    const size_t pts = (size_t)m * sizeof(EdAffine);
    WsCarver cv;
    const auto a_pk = cv.array<EdAffine>(1), a_cards = cv.array<EdAffine>(m), a_e1 = cv.array<EdAffine>(m), a_e2 = cv.array<EdAffine>(m),
               a_diff = cv.array<EdAffine>(m);
    const auto a_proofs = cv.array<uint8_t>((size_t)m * UZK_CP_PROOF_BYTES);
    const auto a_c = cv.array<Fp>(m);
    const auto a_pst = cv.array<uint8_t>((size_t)m * 6), a_ok = cv.array<uint8_t>((size_t)m * 2), a_verdict = cv.array<uint8_t>(m);
    UZK_TRY(cv.reserve(c.ed_ws));
    EdAffine *d_pk = cv(a_pk), *d_cards = cv(a_cards), *d_e1 = cv(a_e1), *d_e2 = cv(a_e2), *d_diff = cv(a_diff);
    uint8_t* d_proofs = cv(a_proofs);
    UZK_HIP(hipMemcpyAsync(d_pk, pk, sizeof(EdAffine), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_cards, cards, pts, hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_e1, e1, pts, hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_e2, e2, pts, hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_proofs, proofs, (size_t)m * UZK_CP_PROOF_BYTES, hipMemcpyHostToDevice, c.stream));
    UZK_LAUNCH(c, "cp_mask_diff", cp_mask_diff_kernel, dim3(ed_grid(m)), dim3(kEdBlock), 0, c.stream, d_e2, d_cards, d_diff, m);
    CpStatement s = {};
    s.g = nullptr; s.h = d_pk; s.u = d_e1; s.v = d_diff;
    s.s_h = 0; s.s_u = s.s_v = 1;
    s.c0 = d_pk; s.c1 = d_cards; s.c2 = d_e1; s.c3 = d_e2;
    s.s_c0 = 0; s.s_c1 = s.s_c2 = s.s_c3 = 1;
    s.n_cls = 4;
    s.label = cp_label_masking();
    return cp_verify_launch(c, s, d_proofs, cv(a_c), cv(a_pst), cv(a_ok), cv(a_verdict), m, verdict_out, challenges_out);
}

int cp_prove_run(Ctx& c, const Fp* sk, const EdAffine* e1, const Fp* omegas, uint32_t m, EdAffine* reveal_out, EdAffine* pk_out, uint8_t* proofs_out,
                 bool anemoi) {
    WsCarver cv;
    const auto a_e1 = cv.array<EdAffine>(m);
    const auto a_om = cv.array<Fp>(m), a_sk = cv.array<Fp>(1);
    const auto a_rv = cv.array<EdAffine>(m), a_ab = cv.array<EdAffine>((size_t)m * 2), a_pk = cv.array<EdAffine>(1);
    const auto a_c = cv.array<Fp>(m);
    const auto a_proofs = cv.array<uint8_t>((size_t)m * UZK_CP_PROOF_BYTES);
    UZK_TRY(cv.reserve(c.ed_ws));
    EdAffine *d_e1 = cv(a_e1), *d_rv = cv(a_rv), *d_ab = cv(a_ab), *d_pk = cv(a_pk);
    Fp *d_om = cv(a_om), *d_sk = cv(a_sk), *d_c = cv(a_c);
    uint8_t* d_proofs = cv(a_proofs);
    UZK_HIP(hipMemcpyAsync(d_e1, e1, (size_t)m * sizeof(EdAffine), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_om, omegas, (size_t)m * sizeof(Fp), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_sk, sk, sizeof(Fp), hipMemcpyHostToDevice, c.stream));
    {
        CpProveArgs a = {};
        a.mask = 0; a.bases = d_e1; a.secret = d_sk; a.omega = d_om; a.out0 = d_rv; a.ab = d_ab; a.extra = d_pk;
        UZK_LAUNCH(c, "cp_prove_mul", cp_prove_mul_kernel, dim3(ed_grid((size_t)m * 3 + 1)), dim3(kEdBlock), 0, c.stream, a, m);
    }
    CpStatement s = {};
    s.g = d_e1; s.h = nullptr; s.u = d_rv; s.v = d_pk;
    s.s_g = s.s_u = 1; s.s_v = 0;
    s.label = cp_label_revealing();
    s.transcript = anemoi ? kCpAnemoi : kCpKeccak;
    UZK_LAUNCH(c, "cp_transcript", cp_transcript_kernel, dim3(ed_grid(m)), dim3(kEdBlock), 0, c.stream, s, nullptr, d_ab, d_c, d_om, d_sk, 0u, d_proofs, m);
    UZK_HIP(hipMemcpyAsync(reveal_out, d_rv, (size_t)m * sizeof(EdAffine), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipMemcpyAsync(pk_out, d_pk, sizeof(EdAffine), hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipMemcpyAsync(proofs_out, d_proofs, (size_t)m * UZK_CP_PROOF_BYTES, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

// pk: one point; cards: m points; rs, omegas: m scalars each
int cp_mask_prove_run(Ctx& c, const EdAffine* pk, const EdAffine* cards, const Fp* rs, const Fp* omegas, uint32_t m, EdAffine* e1_out, EdAffine* e2_out,
                      uint8_t* proofs_out) {
    const size_t pts = (size_t)m * sizeof(EdAffine), scs = (size_t)m * sizeof(Fp);
    WsCarver cv;
    const auto a_pk = cv.array<EdAffine>(1), a_cards = cv.array<EdAffine>(m);
    const auto a_rs = cv.array<Fp>(m), a_om = cv.array<Fp>(m);
    const auto a_e1 = cv.array<EdAffine>(m), a_e2 = cv.array<EdAffine>(m), a_v = cv.array<EdAffine>(m), a_ab = cv.array<EdAffine>((size_t)m * 2);
    const auto a_c = cv.array<Fp>(m);
    const auto a_proofs = cv.array<uint8_t>((size_t)m * UZK_CP_PROOF_BYTES);
    UZK_TRY(cv.reserve(c.ed_ws));
    EdAffine *d_pk = cv(a_pk), *d_cards = cv(a_cards), *d_e1 = cv(a_e1), *d_e2 = cv(a_e2), *d_v = cv(a_v), *d_ab = cv(a_ab);
    Fp *d_rs = cv(a_rs), *d_om = cv(a_om), *d_c = cv(a_c);
    uint8_t* d_proofs = cv(a_proofs);
    UZK_HIP(hipMemcpyAsync(d_pk, pk, sizeof(EdAffine), hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_cards, cards, pts, hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_rs, rs, scs, hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(d_om, omegas, scs, hipMemcpyHostToDevice, c.stream));
    {
        CpProveArgs a = {};
        a.mask = 1; a.bases = d_cards; a.secret = d_rs; a.omega = d_om; a.pk_in = d_pk; a.out0 = d_e1; a.out1 = d_e2; a.ab = d_ab; a.extra = d_v;
        UZK_LAUNCH(c, "cp_prove_mul", cp_prove_mul_kernel, dim3(ed_grid((size_t)m * 5)), dim3(kEdBlock), 0, c.stream, a, m);
    }
    CpStatement s = {};
    s.g = nullptr; s.h = d_pk; s.u = d_e1; s.v = d_v;
    s.s_h = 0; s.s_u = s.s_v = 1;
    s.label = cp_label_masking();
    UZK_LAUNCH(c, "cp_transcript", cp_transcript_kernel, dim3(ed_grid(m)), dim3(kEdBlock), 0, c.stream, s, nullptr, d_ab, d_c, d_om, d_rs, 1u, d_proofs, m);
    UZK_HIP(hipMemcpyAsync(e1_out, d_e1, pts, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipMemcpyAsync(e2_out, d_e2, pts, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipMemcpyAsync(proofs_out, d_proofs, (size_t)m * UZK_CP_PROOF_BYTES, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

// ---- remask keys (process-wide handles) and the remask ---------------------------------------------------------------------------------
struct RemarkEntry {
    int device = 0;
    Fp* d_table = nullptr;             // T_pk
};
static HandleTable<RemarkEntry> g_rk(7ull << 59);
constexpr uint32_t kRemarkTraceChunk = 4096;                        // cards per launch of a remask with trace: 12 KiB of workspace per lane

static void rk_free(const RemarkEntry& e) {
    DeviceGuard on(e.device);
    if (e.d_table) (void)hipFree(e.d_table);
}
static bool rk_lookup(uint64_t h, RemarkEntry* out) { return g_rk.get(h, out); }
bool remark_key_known(uint64_t h, int* device) {
    RemarkEntry e;
    if (!rk_lookup(h, &e)) return false;
    if (device) *device = e.device;
    return true;
}
// T_G of the context: a constant, built by the first call that needs it and kept until the context goes
static int remark_gen_table(Ctx& c, const Fp** out) {
    if (!c.ed_gen_ready) {
        UZK_TRY(c.ed_gen.reserve(kRemarkTableBytes));
        UZK_LAUNCH(c, "remark_table", remark_table_kernel, dim3(ed_grid(kRemarkIters)), dim3(kEdBlock), 0, c.stream, (const EdAffine*)nullptr, c.ed_gen.as<Fp>());
        c.ed_gen_ready = true;
    }
    *out = c.ed_gen.as<Fp>();
    return UZK_OK;
}

int remark_key_create(Ctx& c, const EdAffine* pk, uint64_t* out) {
    const Fp* d_gen = nullptr;
    UZK_TRY(remark_gen_table(c, &d_gen));
    WsCarver cv;
    const auto a_pk = cv.array<EdAffine>(1);
    UZK_TRY(cv.reserve(c.ed_ws));
    EdAffine* d_pk = cv(a_pk);
    RemarkEntry e;
    e.device = c.device;
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&e.d_table), kRemarkTableBytes);
    if (err == hipSuccess) err = hipMemcpyAsync(d_pk, pk, sizeof(EdAffine), hipMemcpyHostToDevice, c.stream);
    if (err == hipSuccess) {
        KernelScope ks(c, "remark_table");
        hipLaunchKernelGGL(remark_table_kernel, dim3(ed_grid(kRemarkIters)), dim3(kEdBlock), 0, c.stream, (const EdAffine*)d_pk, e.d_table);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipStreamSynchronize(c.stream);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        rk_free(e);
        set_error("uzk_remark_key_create: %s", hipGetErrorString(err));
        return UZK_ERR_DEVICE;
    }
    *out = g_rk.insert(e);
    return UZK_OK;
}

// The caller makes sure no remask over this key is still running.
int remark_key_release(uint64_t h) {
    RemarkEntry e;
    if (!g_rk.take(h, &e)) { set_error("uzk_remark_key_release: unknown remask key %llu", (unsigned long long)h); return UZK_ERR_PARAMETER; }
    rk_free(e);
    return UZK_OK;
}

void remark_release_all() { g_rk.drain(rk_free); }

static int rk_for_ctx(Ctx& c, const char* who, uint64_t h, RemarkEntry* e) {
    if (!rk_lookup(h, e)) { set_error("%s: unknown remask key %llu", who, (unsigned long long)h); return UZK_ERR_PARAMETER; }
    if (e->device != c.device) { set_error("%s: the key lives on device %d, the current context on device %d", who, e->device, c.device); return UZK_ERR_PARAMETER; }
    return UZK_OK;
}

int remark_tables_run(Ctx& c, uint64_t h, Fp* pk_tables_out, Fp* gen_tables_out) {
    RemarkEntry e;
    UZK_TRY(rk_for_ctx(c, "uzk_remark_key_tables", h, &e));
    const Fp* d_gen = nullptr;
    UZK_TRY(remark_gen_table(c, &d_gen));
    if (pk_tables_out) UZK_HIP(hipMemcpyAsync(pk_tables_out, e.d_table, kRemarkTableBytes, hipMemcpyDeviceToHost, c.stream));
    if (gen_tables_out) UZK_HIP(hipMemcpyAsync(gen_tables_out, d_gen, kRemarkTableBytes, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

// slot: the output position of every card (the inverse of the caller's perm), or null; trace_out: null or n x 84 x 4 elements
int remark_run(Ctx& c, uint64_t h, const EdAffine* e1, const EdAffine* e2, const uint8_t* digits, const uint32_t* slot, uint32_t n, EdAffine* e1_out,
               EdAffine* e2_out, Fp* trace_out) {
    RemarkEntry e;
    UZK_TRY(rk_for_ctx(c, "uzk_remark_batch", h, &e));
    const Fp* d_gen = nullptr;
    UZK_TRY(remark_gen_table(c, &d_gen));
    const size_t pts = (size_t)n * sizeof(EdAffine), dg = (size_t)n * kRemarkIters;
    const uint32_t chunk = trace_out ? (n < kRemarkTraceChunk ? n : kRemarkTraceChunk) : n;
    const size_t trace_elems = (size_t)kRemarkIters * 4, trace_card = trace_elems * sizeof(Fp), ws_words = (size_t)kRemarkIters * 36;
    WsCarver cv;
    const auto a_e1 = cv.array<EdAffine>(n), a_e2 = cv.array<EdAffine>(n);
    const auto a_dg = cv.array<uint8_t>(dg);
    const auto a_slot = cv.array<uint32_t>(n);
    const auto a_o1 = cv.array<EdAffine>(n), a_o2 = cv.array<EdAffine>(n);
    const auto a_trace = cv.array<Fp>(trace_out ? (size_t)chunk * trace_elems : 0);
    const auto a_ws = cv.array<uint32_t>(trace_out ? 2 * (size_t)chunk * ws_words : 0);
    UZK_TRY(cv.reserve(c.ed_ws));
    RemarkArgs a = {};
    a.t_gen = d_gen; a.t_pk = e.d_table;
    a.e1 = cv(a_e1); a.e2 = cv(a_e2);
    a.digits = cv(a_dg);
    a.slot = slot ? cv(a_slot) : nullptr;
    a.e1_out = cv(a_o1); a.e2_out = cv(a_o2);
    a.trace = trace_out ? cv(a_trace) : nullptr;
    a.ws = cv(a_ws);
    UZK_HIP(hipMemcpyAsync(cv(a_e1), e1, pts, hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(cv(a_e2), e2, pts, hipMemcpyHostToDevice, c.stream));
    UZK_HIP(hipMemcpyAsync(cv(a_dg), digits, dg, hipMemcpyHostToDevice, c.stream));
    if (slot) UZK_HIP(hipMemcpyAsync(cv(a_slot), slot, a_slot.bytes(), hipMemcpyHostToDevice, c.stream));
    for (uint32_t first = 0; first < n; first += chunk) {
        a.first = first; a.count = n - first < chunk ? n - first : chunk;
        UZK_LAUNCH(c, trace_out ? "remark_trace" : "remark", remark_kernel, dim3(ed_grid(2 * (size_t)a.count)), dim3(kEdBlock), 0, c.stream, a);
        if (trace_out) UZK_HIP(hipMemcpyAsync(reinterpret_cast<char*>(trace_out) + first * trace_card, a.trace, a.count * trace_card, hipMemcpyDeviceToHost, c.stream));
    }
    UZK_HIP(hipMemcpyAsync(e1_out, a.e1_out, pts, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipMemcpyAsync(e2_out, a.e2_out, pts, hipMemcpyDeviceToHost, c.stream));
    UZK_HIP(hipStreamSynchronize(c.stream));
    return UZK_OK;
}

int remark_device_tables(Ctx& c, uint64_t h, const Fp** d_pk_out, const Fp** d_gen_out) {
    if (d_pk_out) {                                                // T_G alone needs no key
        RemarkEntry e;
        UZK_TRY(rk_for_ctx(c, "remask tables", h, &e));
        *d_pk_out = e.d_table;
    }
    if (d_gen_out) UZK_TRY(remark_gen_table(c, d_gen_out));
    return UZK_OK;
}

// every array on the device, the trace included: trace[k 84 + i] of card k, the new deck at the cards' slots
int remark_device_run(Ctx& c, uint64_t h, const EdAffine* d_e1, const EdAffine* d_e2, const uint8_t* d_digits, const uint32_t* d_slot, uint32_t n,
                      EdAffine* d_e1_out, EdAffine* d_e2_out, Fp* d_trace) {
    if (n == 0 || n > kRemarkTraceChunk) { set_error("remask on the device: %u cards (1 .. %u per call)", n, kRemarkTraceChunk); return UZK_ERR_PARAMETER; }
    RemarkArgs a = {};
    UZK_TRY(remark_device_tables(c, h, &a.t_pk, &a.t_gen));
    WsCarver cv;
    const auto a_ws = cv.array<uint32_t>(2 * (size_t)n * kRemarkIters * 36);
    UZK_TRY(cv.reserve(c.ed_ws));
    a.e1 = d_e1; a.e2 = d_e2; a.digits = d_digits; a.slot = d_slot;
    a.e1_out = d_e1_out; a.e2_out = d_e2_out; a.trace = d_trace; a.ws = cv(a_ws);
    a.first = 0; a.count = n;
    UZK_LAUNCH(c, "remark_trace", remark_kernel, dim3(ed_grid(2 * (size_t)n)), dim3(kEdBlock), 0, c.stream, a);
    return UZK_OK;
}

// n records of EdRawIn (72 words) -> n records of EdRawOut (37 words), both on the host
int ed_raw_op_device(Ctx& c, int op, const uint32_t* in, uint32_t* out, size_t n) {
    if (n == 0) return UZK_OK;
    static_assert(sizeof(EdRawIn) == 72 * sizeof(uint32_t) && sizeof(EdRawOut) == 37 * sizeof(uint32_t), "records are packed words");
    EdRawIn* din = nullptr;
    EdRawOut* dout = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&din), n * sizeof(EdRawIn));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&dout), n * sizeof(EdRawOut));
    if (e == hipSuccess) e = hipMemcpyAsync(din, in, n * sizeof(EdRawIn), hipMemcpyHostToDevice, c.stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(ed_raw_kat_kernel, dim3(ed_grid(n)), dim3(kEdBlock), 0, c.stream, op, din, dout, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, n * sizeof(EdRawOut), hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    UZK_HIP(e);
    return UZK_OK;
}

}  // namespace uzk
