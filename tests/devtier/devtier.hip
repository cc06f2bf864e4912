// TEST INFRASTRUCTURE: the device tier.  Applies one ZKP_HD function of the product's math headers to n independent cases whose operands are
// RAW LIMBS in the type's own layout (so a test can place every limb at the bound the header promises), either in a host loop or in one
// launch with one lane per case, and returns raw result limbs plus the type's own canonicalising store.  Compiled with the product's
// flags for gfx950, so the device leg checks the code generation the product ships with (mul64wide's __umul64hi branch, the v_mad_u64_u32
// chains); the host leg lets the case lists and bigint references be checked without a GPU.  Not part of the product library.
// Cases, references and the op tables that mirror the switch statements below: tests/devtier_cases.py.
#include "../../libzkp_amd/csrc/fe25519.h"
#include "../../libzkp_amd/csrc/bn254_fq.h"
#include "../../libzkp_amd/csrc/bn254_fq9.h"
#include "../../libzkp_amd/csrc/bn254_fr9.h"
#include "../../libzkp_amd/csrc/bn254_g.h"
#include "../../libzkp_amd/csrc/stark_steps.h"
#include "../../libzkp_amd/csrc/g16_launch.h"
#include "../../libzkp_amd/csrc/edg_launch.h"
#include "devtier_family.h"
#include <algorithm>
#include <vector>
using namespace zkp;
using namespace devtier;             // Shape, ld, st, run_family: shared with devtier_pairing.hip

namespace {

// ------------------------------------------------------------------------------------------------ fe25519: ten 25.5-bit limbs
// result: 10 raw limbs, 8 canonical words (fe_towords), 1 flag
struct FeCase {
    ZKP_HD static Shape shape(int op) {
        switch (op) {
            case 0: case 2: case 3: case 9: return Shape{10, 10, 0, 19};
            case 1: case 4: case 5: case 6: case 7: case 8: return Shape{10, 0, 0, 19};
            default: return Shape{0, 0, 0, 0};
        }
    }
    ZKP_HD static void run(int op, const uint32_t* a, const uint32_t* b, const uint32_t*, uint32_t* out) {
        const fe x = ld<fe, 10>(a);
        fe r = x; uint32_t flag = 0;
        switch (op) {
            case 0: r = fe_mul(x, ld<fe, 10>(b)); break;
            case 1: r = fe_sq(x); break;
            case 2: r = fe_add(x, ld<fe, 10>(b)); break;
            case 3: r = fe_sub(x, ld<fe, 10>(b)); break;
            case 4: r = fe_neg(x); break;
            case 5: r = fe_carry(x); break;
            case 6: r = fe_abs(x); break;
            case 7: break;                                  // fe_towords of the operand itself
            case 8: r = fe_pow22523(x); break;
            default: flag = fe_sqrt_ratio_m1(r, x, ld<fe, 10>(b)) ? 1u : 0u; break;
        }
        st<fe, 10>(out, r);
        fe_towords(out + 10, r);
        out[18] = flag;
    }
};

// ------------------------------------------------------------------------------------------------ bn254 fq: ten 26-bit limbs
// result: 10 raw limbs, 8 canonical words (fq_to_raw: value / 2^260 mod p); fq_eq and fq_is_zero return their flag in word 0 (words 1..9 zero)
// and the canonical words of their first operand
struct FqCase {
    ZKP_HD static Shape shape(int op) {
        switch (op) {
            case 0: case 3: case 5: case 6: case 7: case 12: case 13: case 17: return Shape{10, 10, 0, 18};
            case 1: case 4: case 8: case 9: case 10: case 11: case 14: case 15: case 18: return Shape{10, 0, 0, 18};
            case 2: return Shape{20, 20, 0, 18};
            case 16: return Shape{8, 0, 0, 18};
            default: return Shape{0, 0, 0, 0};
        }
    }
    ZKP_HD static void run(int op, const uint32_t* a, const uint32_t* b, const uint32_t*, uint32_t* out) {
        const fq x = op == 16 ? fq_zero() : ld<fq, 10>(a);  // (16 takes eight words, not ten limbs)
        fq r = x;
        switch (op) {
            case 0: r = fq_mul(x, ld<fq, 10>(b)); break;
            case 1: r = fq_sq(x); break;
            case 2: r = fq_mul_add2(x, ld<fq, 10>(a + 10), ld<fq, 10>(b), ld<fq, 10>(b + 10)); break;
            case 3: r = fq_add_l(x, ld<fq, 10>(b)); break;
            case 4: r = fq_dbl_l(x); break;
            case 5: r = fq_sub_k4(x, ld<fq, 10>(b)); break;
            case 6: r = fq_sub_k8(x, ld<fq, 10>(b)); break;
            case 7: r = fq_sub_k16(x, ld<fq, 10>(b)); break;
            case 8: r = fq_reduce_weak(x); break;
            case 9: r = fq_carry(x); break;
            case 10: break;                                 // fq_to_raw of the operand itself
            case 11: r = fq_inv(x); break;
            // the "safe" (always reduced) operations and the two predicates the verdict kernels use
            case 12: r = fq_add(x, ld<fq, 10>(b)); break;
            case 13: r = fq_sub(x, ld<fq, 10>(b)); break;
            case 14: r = fq_neg(x); break;
            case 15: r = fq_dbl(x); break;
            case 16: r = fq_from_raw(a); break;
            default: {                                      // 17 fq_eq, 18 fq_is_zero
                const bool flag = op == 17 ? fq_eq(x, ld<fq, 10>(b)) : fq_is_zero(x);
                ZKP_UNROLL for (int i = 0; i < 10; i++) out[i] = 0;
                out[0] = flag ? 1u : 0u;
                fq_to_raw(out + 10, x);
                return;
            }
        }
        st<fq, 10>(out, r);
        fq_to_raw(out + 10, r);
    }
};

// ------------------------------------------------------------------------------------------------ bn254 fq9: nine 29-bit limbs
// result: 10 words of raw limbs (nine for an fq9, ten for an fq; unused words zero), 8 canonical words (value / 2^261 mod p for an
// fq9 result through fq9_to_fq and fq_to_raw, value / 2^260 mod p for an fq result; for pack8 the packed words themselves)
struct Fq9Case {
    ZKP_HD static Shape shape(int op) {
        switch (op) {
            case 0: case 4: case 5: case 6: case 7: case 12: return Shape{9, 9, 0, 18};
            case 1: case 13: case 14: case 15: case 16: case 18: case 19: case 22: return Shape{9, 0, 0, 18};
            case 2: case 11: return Shape{18, 18, 0, 18};
            case 3: return Shape{36, 36, 0, 18};
            case 8: return Shape{9, 9, 1, 18};
            case 9: case 10: return Shape{18, 9, 0, 18};
            case 17: case 21: return Shape{10, 0, 0, 18};
            case 20: return Shape{8, 0, 0, 18};
            default: return Shape{0, 0, 0, 0};
        }
    }
    ZKP_HD static void run(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out) {
        ZKP_UNROLL for (int i = 0; i < 18; i++) out[i] = 0;
        const fq9 x = ld<fq9, 9>(a);
        fq9 r = x;
        switch (op) {
            case 0: r = fq9_mul(x, ld<fq9, 9>(b)); break;
            case 1: r = fq9_sq(x); break;
            case 2: case 11: r = fq9_mul_add2(x, ld<fq9, 9>(a + 9), ld<fq9, 9>(b), ld<fq9, 9>(b + 9)); break;   // 11: the loose operands of g1_mmadd9's Y3
            case 3: r = fq9_mul_add4(x, ld<fq9, 9>(a + 9), ld<fq9, 9>(a + 18), ld<fq9, 9>(a + 27), ld<fq9, 9>(b), ld<fq9, 9>(b + 9), ld<fq9, 9>(b + 18), ld<fq9, 9>(b + 27)); break;
            case 4: r = fq9_add(x, ld<fq9, 9>(b)); break;
            case 5: r = fq9_sub_k<4>(x, ld<fq9, 9>(b)); break;
            case 6: r = fq9_sub_k<8>(x, ld<fq9, 9>(b)); break;
            case 7: r = fq9_sub_k<16>(x, ld<fq9, 9>(b)); break;
            case 8: r = fq9_sgn_sub_k<8>(c[0] != 0, x, ld<fq9, 9>(b)); break;
            case 9: r = fq9_sub2_k<4>(x, ld<fq9, 9>(a + 9), ld<fq9, 9>(b)); break;
            case 10: r = fq9_sub2_k<8>(x, ld<fq9, 9>(a + 9), ld<fq9, 9>(b)); break;
            case 12: r = fq9_sub_loose<8>(x, ld<fq9, 9>(b)); break;
            case 13: r = fq9_neg_loose<4>(x); break;
            case 14: r = fq9_neg_k<4>(x); break;
            case 15: r = fq9_neg_k<32>(x); break;
            case 16: r = fq9_dbl_l(x); break;
            case 17: r = fq9_reslice(ld<fq, 10>(a)); break;
            case 18: { const fq t = fq_reslice(x); st<fq, 10>(out, t); fq_to_raw(out + 10, t); return; }
            case 19: st<fq9, 9>(out, x); fq9_pack8(out + 10, x); return;
            case 20: r = fq9_unpack8(a); break;
            case 21: r = fq9_from_fq(ld<fq, 10>(a)); break;
            default: { const fq t = fq9_to_fq(x); st<fq, 10>(out, t); fq_to_raw(out + 10, t); return; }      // 22
        }
        st<fq9, 9>(out, r);
        // the canonical store of the nine-limb form is the way the product leaves it: one product with 2^260 mod p, re-slice, reduce.
        // It takes carried9 operands, so ops whose results are loose on purpose (12, 13, 16) are carried first.
        fq9 cr = r;
        if (op == 12 || op == 13 || op == 16) cr = fq9_add(r, fq9_zero());
        fq_to_raw(out + 10, fq9_to_fq(cr));
    }
};

// ------------------------------------------------------------------------------------------------ bn254 fr9: nine 29-bit limbs mod r
// result: 9 raw limbs, 8 words: fr9_to_fr (value / 2^261 * 2^256 mod r, below 2r, NOT canonicalised: the header's own store)
struct Fr9Case {
    ZKP_HD static Shape shape(int op) {
        switch (op) {
            case 0: case 1: case 2: return Shape{9, 9, 0, 17};
            case 3: case 5: return Shape{9, 0, 0, 17};
            case 4: return Shape{8, 0, 0, 17};
            default: return Shape{0, 0, 0, 0};
        }
    }
    ZKP_HD static void run(int op, const uint32_t* a, const uint32_t* b, const uint32_t*, uint32_t* out) {
        fr9 r;
        switch (op) {
            case 0: r = fr9_mul(ld<fr9, 9>(a), ld<fr9, 9>(b)); break;
            case 1: r = fr9_add(ld<fr9, 9>(a), ld<fr9, 9>(b)); break;
            case 2: r = fr9_sub_k<2>(ld<fr9, 9>(a), ld<fr9, 9>(b)); break;
            case 3: r = fr9_reduce_weak(ld<fr9, 9>(a)); break;
            case 4: r = fr9_from_fr(ld<Fp<FrParams>, 8>(a)); break;
            default: r = ld<fr9, 9>(a); break;              // 5: fr9_to_fr of the operand itself
        }
        st<fr9, 9>(out, r);
        st<Fp<FrParams>, 8>(out + 9, fr9_to_fr<FrParams>(r));
    }
};

// ------------------------------------------------------------------------------------------------ f128: two 64-bit words, canonical in and out
struct F128Case {
    ZKP_HD static Shape shape(int op) {
        switch (op) {
            case 0: case 1: case 2: return Shape{4, 4, 0, 4};
            case 3: return Shape{4, 0, 0, 4};
            default: return Shape{0, 0, 0, 0};
        }
    }
    ZKP_HD static f128 get(const uint32_t* w) { return f128_make((uint64_t)w[0] | ((uint64_t)w[1] << 32), (uint64_t)w[2] | ((uint64_t)w[3] << 32)); }
    ZKP_HD static void run(int op, const uint32_t* a, const uint32_t* b, const uint32_t*, uint32_t* out) {
        const f128 x = get(a);
        f128 r;
        switch (op) {
            case 0: r = f128_mul(x, get(b)); break;
            case 1: r = f128_add(x, get(b)); break;
            case 2: r = f128_sub(x, get(b)); break;
            default: r = f128_neg(x); break;
        }
        f128_words(out, r);
    }
};

// ------------------------------------------------------------------------------------------------ the MSM loops' point steps
// a: the accumulator's coordinates as raw limbs; b: the table entry (x, y); c: one word, the digit's sign (1 = negative).  A negative
// digit is applied the way the kernel applies it (msm_kernel.h's Msm structs): y -> 4p - y before the step for G1, the step's own
// `negate` for G2.  Result: the accumulator after the step, raw limbs, then the affine point it denotes as canonical words (through
// the product's own conversion back to Jacobian and jac_to_aff) and a word that is 1 for infinity.
struct PointCase {
    ZKP_HD static Shape shape(int op) {
        switch (op) {
            case 0: return Shape{30, 20, 1, 30 + 17};       // g1_madd_lazy   Jac<fq>
            case 1: return Shape{40, 20, 1, 40 + 17};       // g1_mmadd_lazy  g1_xyzz
            case 2: return Shape{36, 18, 1, 36 + 17};       // g1_mmadd9      g1_xyzz9
            case 3: return Shape{60, 40, 1, 60 + 33};       // g2_madd_lazy   Jac<fq2>
            case 4: return Shape{72, 36, 1, 72 + 33};       // g2_mmadd9      g2_xyzz9
            default: return Shape{0, 0, 0, 0};
        }
    }
    ZKP_HD static void aff1(uint32_t* out, const Jac<fq>& j) {
        g1_aff p; const bool fin = jac_to_aff(p, j);
        ZKP_UNROLL for (int i = 0; i < 16; i++) out[i] = 0;
        if (fin) { fq_to_raw(out, p.x); fq_to_raw(out + 8, p.y); }
        out[16] = fin ? 0u : 1u;
    }
    ZKP_HD static void aff2(uint32_t* out, const Jac<fq2>& j) {
        g2_aff p; const bool fin = jac_to_aff(p, j);
        ZKP_UNROLL for (int i = 0; i < 32; i++) out[i] = 0;
        if (fin) { fq_to_raw(out, p.x.c0); fq_to_raw(out + 8, p.x.c1); fq_to_raw(out + 16, p.y.c0); fq_to_raw(out + 24, p.y.c1); }
        out[32] = fin ? 0u : 1u;
    }
    ZKP_HD static void run(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out) {
        const bool neg = c[0] != 0;
        switch (op) {
            case 0: {
                const Jac<fq> p{ld<fq, 10>(a), ld<fq, 10>(a + 10), ld<fq, 10>(a + 20)};
                Aff<fq> q{ld<fq, 10>(b), ld<fq, 10>(b + 10)};
                if (neg) q.y = fq_sub_k4(fq_zero(), q.y);
                const Jac<fq> r = g1_madd_lazy(p, q);
                st<fq, 10>(out, r.X); st<fq, 10>(out + 10, r.Y); st<fq, 10>(out + 20, r.Z);
                aff1(out + 30, r); break;
            }
            case 1: {
                const g1_xyzz p{ld<fq, 10>(a), ld<fq, 10>(a + 10), ld<fq, 10>(a + 20), ld<fq, 10>(a + 30)};
                Aff<fq> q{ld<fq, 10>(b), ld<fq, 10>(b + 10)};
                if (neg) q.y = fq_sub_k4(fq_zero(), q.y);
                const g1_xyzz r = g1_mmadd_lazy(p, q);
                st<fq, 10>(out, r.X); st<fq, 10>(out + 10, r.Y); st<fq, 10>(out + 20, r.ZZ); st<fq, 10>(out + 30, r.ZZZ);
                aff1(out + 40, jac_from_xyzz(r)); break;
            }
            case 2: {
                const g1_xyzz9 p{ld<fq9, 9>(a), ld<fq9, 9>(a + 9), ld<fq9, 9>(a + 18), ld<fq9, 9>(a + 27)};
                g1_aff9 q{ld<fq9, 9>(b), ld<fq9, 9>(b + 9)};
                if (neg) q.y = fq9_neg_k<4>(q.y);
                const g1_xyzz9 r = g1_mmadd9(p, q);
                st<fq9, 9>(out, r.X); st<fq9, 9>(out + 9, r.Y); st<fq9, 9>(out + 18, r.ZZ); st<fq9, 9>(out + 27, r.ZZZ);
                aff1(out + 36, jac_from_xyzz9(r)); break;
            }
            case 3: {
                const Jac<fq2> p{fq2{ld<fq, 10>(a), ld<fq, 10>(a + 10)}, fq2{ld<fq, 10>(a + 20), ld<fq, 10>(a + 30)}, fq2{ld<fq, 10>(a + 40), ld<fq, 10>(a + 50)}};
                const Aff<fq2> q{fq2{ld<fq, 10>(b), ld<fq, 10>(b + 10)}, fq2{ld<fq, 10>(b + 20), ld<fq, 10>(b + 30)}};
                const Jac<fq2> r = g2_madd_lazy(p, q, neg);
                st<fq, 10>(out, r.X.c0); st<fq, 10>(out + 10, r.X.c1); st<fq, 10>(out + 20, r.Y.c0); st<fq, 10>(out + 30, r.Y.c1); st<fq, 10>(out + 40, r.Z.c0); st<fq, 10>(out + 50, r.Z.c1);
                aff2(out + 60, r); break;
            }
            default: {
                g2_xyzz9 p; fq2_9* pc[4] = {&p.X, &p.Y, &p.ZZ, &p.ZZZ};
                ZKP_UNROLL for (int k = 0; k < 4; k++) { pc[k]->c0 = ld<fq9, 9>(a + 18 * k); pc[k]->c1 = ld<fq9, 9>(a + 18 * k + 9); }
                const g2_aff9 q{fq2_9{ld<fq9, 9>(b), ld<fq9, 9>(b + 9)}, fq2_9{ld<fq9, 9>(b + 18), ld<fq9, 9>(b + 27)}};
                const g2_xyzz9 r = g2_mmadd9(p, q, neg);
                const fq2_9* rc[4] = {&r.X, &r.Y, &r.ZZ, &r.ZZZ};
                ZKP_UNROLL for (int k = 0; k < 4; k++) { st<fq9, 9>(out + 18 * k, rc[k]->c0); st<fq9, 9>(out + 18 * k + 9, rc[k]->c1); }
                aff2(out + 72, jac_from_g2_xyzz9(r)); break;
            }
        }
    }
};

// ------------------------------------------------------------------------------------------------ sc25519: eight 32-bit words, Montgomery form
// result: 16 words -- the result's eight words and sc_to_raw of it; the recodings return their packed digit words (13 / 8) instead
struct ScCase {
    ZKP_HD static Shape shape(int op) {
        switch (op) {
            case 0: case 1: case 2: return Shape{8, 8, 0, 16};
            case 3: case 4: case 5: case 7: case 8: case 9: case 10: return Shape{8, 0, 0, 16};
            case 6: return Shape{16, 0, 0, 16};
            default: return Shape{0, 0, 0, 0};
        }
    }
    ZKP_HD static void run(int op, const uint32_t* a, const uint32_t* b, const uint32_t*, uint32_t* out) {
        ZKP_UNROLL for (int i = 0; i < 16; i++) out[i] = 0;
        const sc x = ld<sc, 8>(a);
        sc r = x;
        switch (op) {
            case 0: r = sc_mul(x, ld<sc, 8>(b)); break;
            case 1: r = sc_add(x, ld<sc, 8>(b)); break;
            case 2: r = sc_sub(x, ld<sc, 8>(b)); break;
            case 3: r = sc_neg(x); break;
            case 4: r = sc_invert(x); break;
            case 5: r = sc_invert_fermat(x); break;
            case 6: r = sc_from_wide(a); break;
            case 7: sc_recode_signed1024(out, x); return;
            case 8: sc_recode_signed65536(out, x); return;
            case 9: r = sc_from_raw256(x); break;
            default: break;                                 // 10: sc_to_raw of the operand itself
        }
        st<sc, 8>(out, r);
        st<sc, 8>(out + 8, sc_to_raw(r));
    }
};

// ------------------------------------------------------------------------------------------------ Fp<FrParams>: eight 32-bit words, Montgomery form, values below 2r
// result: 16 words -- the result's eight words and fp_to_raw of it; fr_glv_split returns mag1[4], neg1, mag2[4], neg2
struct FpCase {
    ZKP_HD static Shape shape(int op) {
        switch (op) {
            case 0: case 1: case 2: return Shape{8, 8, 0, 16};
            case 3: case 4: case 6: case 7: case 8: return Shape{8, 0, 0, 16};
            case 5: return Shape{16, 0, 0, 16};
            default: return Shape{0, 0, 0, 0};
        }
    }
    ZKP_HD static void run(int op, const uint32_t* a, const uint32_t* b, const uint32_t*, uint32_t* out) {
        ZKP_UNROLL for (int i = 0; i < 16; i++) out[i] = 0;
        const fr x = ld<fr, 8>(a);
        fr r = x;
        switch (op) {
            case 0: r = fp_mul(x, ld<fr, 8>(b)); break;
            case 1: r = fp_add(x, ld<fr, 8>(b)); break;
            case 2: r = fp_sub(x, ld<fr, 8>(b)); break;
            case 3: r = fp_neg(x); break;
            case 4: r = fp_inv(x); break;
            case 5: r = fp_from_wide<FrParams>(a); break;
            case 6: {
                glv_half h1, h2; fr_glv_split(a, h1, h2);
                ZKP_UNROLL for (int i = 0; i < 4; i++) { out[i] = h1.mag[i]; out[5 + i] = h2.mag[i]; }
                out[4] = h1.neg ? 1u : 0u; out[9] = h2.neg ? 1u : 0u;
                return;
            }
            case 7: r = fp_from_raw<FrParams>(a); break;
            default: break;                                 // 8: fp_to_raw of the operand itself
        }
        st<fr, 8>(out, r);
        fp_to_raw(out + 8, r);
    }
};

// ------------------------------------------------------------------------------------------------ ed25519 group steps (complete formulas)
// a: the point (X, Y, Z, T), 40 limbs; b: the other operand -- affine Niels limbs (30), an extended point (40) or a packed table entry (24
// words); c: the digit's sign for edg_accumulate.  result: the point's 40 raw limbs and ge_ristretto_encode of it
struct GeCase {
    ZKP_HD static Shape shape(int op) {
        switch (op) {
            case 0: return Shape{40, 30, 0, 48};
            case 1: return Shape{40, 40, 0, 48};
            case 2: case 4: return Shape{40, 0, 0, 48};
            case 3: return Shape{40, 24, 1, 48};
            default: return Shape{0, 0, 0, 0};
        }
    }
    ZKP_HD static ge point(const uint32_t* w) { return ge{ld<fe, 10>(w), ld<fe, 10>(w + 10), ld<fe, 10>(w + 20), ld<fe, 10>(w + 30)}; }
    ZKP_HD static void run(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out) {
        const ge p = point(a);
        ge r = p;
        switch (op) {
            case 0: r = ge_madd(p, ge_niels{ld<fe, 10>(b), ld<fe, 10>(b + 10), ld<fe, 10>(b + 20)}); break;
            case 1: r = ge_add(p, point(b)); break;
            case 2: r = ge_dbl(p); break;
            case 3: r = edg_accumulate(p, c[0] ? -1 : 1, b); break;
            default: break;                                 // 4: ge_ristretto_encode of the operand itself
        }
        st<fe, 10>(out, r.X); st<fe, 10>(out + 10, r.Y); st<fe, 10>(out + 20, r.Z); st<fe, 10>(out + 30, r.T);
        ge_ristretto_encode(out + 40, r);
    }
};

// ------------------------------------------------------------------------------------------------ the gather and sum kernels, driven directly
// The launchers are the product's own (g16_launch.h, edg_launch.h, linked from libzkp_hip.so), so the code object under test is the shipped
// one; the views are synthetic.  Points come in and go out as canonical affine words (G1: x | y, 16 words; G2: x.c0 | x.c1 | y.c0 | y.c1,
// 32 words; ed25519: x | y, 16 words) plus, on the way out, one word that is 1 for the neutral element (2: an ed25519 T that is not X Y / Z).
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4); }
    hipError_t put(const void* src, size_t bytes) { const hipError_t e = alloc(bytes); return e != hipSuccess || !bytes ? e : hipMemcpy(p, src, bytes, hipMemcpyHostToDevice); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// affine words (+ the neutral flag) -> a Jacobian representative with Z = z (never 1 for z != 1)
template <class F> struct BnField;
template <> struct BnField<fq> {
    static fq coord(const uint32_t* w) { return fq_from_raw(w); }
    static fq small(uint64_t x) { return fq_from_u64(x); }
};
template <> struct BnField<fq2> {
    static fq2 coord(const uint32_t* w) { return fq2{fq_from_raw(w), fq_from_raw(w + 8)}; }
    static fq2 small(uint64_t x) { return fq2{fq_from_u64(x), fq_from_u64(x + 1)}; }
};
template <class F> Jac<F> jac_of(const uint32_t* w, uint32_t aff_w, bool neutral, uint64_t z) {
    if (neutral) return jac_infinity<F>();
    const F zf = BnField<F>::small(z), zz = f_sq(zf);
    return Jac<F>{f_mul(BnField<F>::coord(w), zz), f_mul(BnField<F>::coord(w + aff_w / 2), f_mul(zz, zf)), zf};
}
// one point type of the two kernels: its words, the stored form of a table entry and of an accumulator, its launchers
struct BnG1 {
    static constexpr uint32_t AFF_W = 16, ACC_W = G1_JAC_W, ENTRY_W = 16;
    static void entry(uint32_t* e, const uint32_t* w) { fq9_pack8(e, fq9_from_fq(fq_from_raw(w))); fq9_pack8(e + 8, fq9_from_fq(fq_from_raw(w + 8))); }      // what k_g16_build_table stores
    static void store(uint32_t* p, uint32_t idx, uint32_t row, uint32_t rows, const uint32_t* w, bool neutral, uint64_t z) { st_g1_jac(p, idx, row, rows, jac_of<fq>(w, AFF_W, neutral, z)); }
    static void words(uint32_t* out, const uint32_t* p, uint32_t idx, uint32_t row, uint32_t rows) { PointCase::aff1(out, ld_g1_jac(p, idx, row, rows)); }
    static void launch_msm(const MsmView& m, bool) { g16_launch_msm(false, m, nullptr); }
    static void launch_sum(const ReduceView& R, uint32_t* sums) { g16_launch_sum(false, R, sums, nullptr); }
};
struct BnG2 {
    static constexpr uint32_t AFF_W = 32, ACC_W = G2_JAC_W, ENTRY_W = 32;
    static void entry(uint32_t* e, const uint32_t* w) { for (int k = 0; k < 4; k++) fq9_pack8(e + 8 * k, fq9_from_fq(fq_from_raw(w + 8 * k))); }
    static void store(uint32_t* p, uint32_t idx, uint32_t row, uint32_t rows, const uint32_t* w, bool neutral, uint64_t z) { st_g2_jac(p, idx, row, rows, jac_of<fq2>(w, AFF_W, neutral, z)); }
    static void words(uint32_t* out, const uint32_t* p, uint32_t idx, uint32_t row, uint32_t rows) { PointCase::aff2(out, ld_g2_jac(p, idx, row, rows)); }
    static void launch_msm(const MsmView& m, bool) { g16_launch_msm(true, m, nullptr); }
    static void launch_sum(const ReduceView& R, uint32_t* sums) { g16_launch_sum(true, R, sums, nullptr); }
};
struct Ed {
    static constexpr uint32_t AFF_W = 16, ACC_W = GE_W, ENTRY_W = EDG_SLOT_W;
    static ge point(const uint32_t* w, bool neutral, uint64_t z) {                 // (x z, y z, z, x y z)
        const uint32_t zw[8] = {(uint32_t)z, 0, 0, 0, 0, 0, 0, 0};
        const fe zf = fe_fromwords(zw);
        if (neutral) return ge{fe_zero(), zf, zf, fe_zero()};
        const fe x = fe_fromwords(w), y = fe_fromwords(w + 8);
        return ge{fe_mul(x, zf), fe_mul(y, zf), zf, fe_mul(fe_mul(x, y), zf)};
    }
    // the table builder's own last step (edg_step_affine: eight projective slots to packed affine Niels with one inversion) on a group of
    // eight copies of the point; slot 0 is the entry
    static void entry(uint32_t* e, const uint32_t* w) {
        uint32_t grp[EDG_INV * EDG_SLOT_W];
        const ge p = point(w, false, 3);
        for (uint32_t i = 0; i < EDG_INV; i++) { uint32_t* q = grp + i * EDG_SLOT_W; for (int k = 0; k < 10; k++) { q[k] = p.X.v[k]; q[10 + k] = p.Y.v[k]; q[20 + k] = p.Z.v[k]; } q[30] = q[31] = 0; }
        edg_step_affine(grp, 0);
        for (uint32_t k = 0; k < EDG_SLOT_W; k++) e[k] = grp[k];
    }
    static void store(uint32_t* p, uint32_t idx, uint32_t row, uint32_t rows, const uint32_t* w, bool neutral, uint64_t z) { st_ge(p, idx, row, rows, point(w, neutral, z)); }
    static void words(uint32_t* out, const uint32_t* p, uint32_t idx, uint32_t row, uint32_t rows) {
        const ge g = ld_ge(p, idx, row, rows);
        const fe zi = edg_fe_invert(g.Z), x = fe_mul(g.X, zi), y = fe_mul(g.Y, zi);
        fe_towords(out, x); fe_towords(out + 8, y);
        const bool neutral = fe_iszero(x) && fe_eq(y, fe_one());
        out[16] = !fe_eq(fe_mul(g.T, g.Z), fe_mul(g.X, g.Y)) || fe_iszero(g.Z) ? 2u : neutral ? 1u : 0u;
        if (neutral) for (int i = 0; i < 16; i++) out[i] = 0;
    }
    static void launch_msm(const MsmView& m, bool raised) { const uint32_t ngroups = (m.rows + 255u) / 256u; edg_launch_msm(m, ngroups, m.nchunks * ngroups, nullptr, raised); }
    static void launch_sum(const ReduceView& R, uint32_t* sums) { edg_launch_sum(R, sums, nullptr); }
};

// error codes below zero: the view would send the kernel outside what was allocated or populated, and nothing was launched
template <class B> int run_msm(bool raised, uint32_t rows, uint32_t nchunks, uint32_t nsteps, const uint32_t* steps, const uint32_t* chunk_step0, const uint32_t* digits, uint32_t digit_rows,
                               const uint32_t* points, const uint64_t* point_slot, uint32_t npoints, uint64_t table_entries, const uint32_t* acc_init, uint32_t* out) {
    if (!rows || !nchunks || rows > (1u << 16) || nchunks > (1u << 12) || !chunk_step0 || !out || (nsteps && (!steps || !digits)) || (npoints && (!points || !point_slot))) return -1;
    if (table_entries > (1ull << 28)) return -1;
    std::vector<uint64_t> populated(point_slot, point_slot + npoints);
    std::sort(populated.begin(), populated.end());
    for (uint32_t i = 0; i < npoints; i++) if (point_slot[i] >= table_entries) return -2;
    if (chunk_step0[0] != 0) return -3;
    for (uint32_t c = 0; c < nchunks; c++) if (chunk_step0[c + 1] < chunk_step0[c] || chunk_step0[c + 1] > nsteps) return -3;
    // Only the half of a digit word that a step selects is checked: the kernel decodes that half alone (T::digit(word, ds.y & 1)), so the
    // other half never becomes an entry index.  That every entry a lane can fetch is inside the allocation AND was written by the test is
    // what makes the never-cleared table safe to read.
    for (uint32_t t = 0; t < chunk_step0[nchunks]; t++) {
        const uint32_t wrow = steps[2 * t + 1] >> 1, half = steps[2 * t + 1] & 1u;
        if (wrow >= digit_rows) return -4;                                  // a digit row outside the digit buffer
        for (uint32_t r = 0; r < rows; r++) {
            const int32_t d = (int32_t)(int16_t)(digits[(size_t)wrow * rows + r] >> (16 * half));
            if (d == 0) continue;
            const uint64_t idx = (uint64_t)steps[2 * t] + (uint32_t)((d < 0 ? -d : d) - 1);
            if (idx >= table_entries) return -5;                            // an entry outside the allocated table
            if (!std::binary_search(populated.begin(), populated.end(), idx)) return -6;      // ... or one the test never wrote
        }
    }
    DevBuf table, dsteps, dstep0, ddigits, dacc, dpartial;
    hipError_t e = table.alloc((size_t)table_entries * B::ENTRY_W * 4);     // allocated, never cleared: only the populated entries are written
    for (uint32_t i = 0; i < npoints && e == hipSuccess; i++) {
        uint32_t ent[B::ENTRY_W]; B::entry(ent, points + (size_t)i * B::AFF_W);
        e = hipMemcpy(table.as<uint32_t>() + (size_t)point_slot[i] * B::ENTRY_W, ent, sizeof ent, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = dsteps.put(steps, (size_t)nsteps * 8);
    if (e == hipSuccess) e = dstep0.put(chunk_step0, (size_t)(nchunks + 1) * 4);
    if (e == hipSuccess) e = ddigits.put(digits, (size_t)digit_rows * rows * 4);
    if (e == hipSuccess && acc_init) {
        uint32_t a[B::ACC_W]; B::store(a, 0, 0, 1, acc_init, false, 5);
        e = dacc.put(a, sizeof a);
    }
    const size_t pwords = (size_t)nchunks * B::ACC_W * rows;
    if (e == hipSuccess) e = dpartial.alloc(pwords * 4);
    if (e == hipSuccess) e = hipMemset(dpartial.p, 0xA5, pwords * 4);       // a (chunk, row) the kernel leaves out is seen
    if (e != hipSuccess) return (int)e;
    MsmView m{};
    m.rows = rows; m.nchunks = nchunks; m.table = table.as<uint32_t>(); m.digits = ddigits.as<uint32_t>(); m.partial = dpartial.as<uint32_t>();
    m.acc_init = acc_init ? dacc.as<uint32_t>() : nullptr; m.steps = dsteps.as<uint32_t>(); m.chunk_step0 = dstep0.as<uint32_t>();
    B::launch_msm(m, raised);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    std::vector<uint32_t> part(pwords);
    if (e == hipSuccess) e = hipMemcpy(part.data(), dpartial.p, pwords * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;
    for (uint32_t c = 0; c < nchunks; c++)
        for (uint32_t r = 0; r < rows; r++) B::words(out + ((size_t)c * rows + r) * (B::AFF_W + 1), part.data(), c, r, rows);
    return 0;
}

template <class B> int run_sum(uint32_t rows, uint32_t nchunks, uint32_t ntargets, const uint16_t* begin, const uint16_t* end, const uint32_t* partial, const uint32_t* corr, uint32_t* out) {
    if (!rows || !ntargets || rows > (1u << 12) || nchunks > (1u << 12) || ntargets > (1u << 10) || !begin || !out || (nchunks && !partial)) return -1;
    for (uint32_t t = 0; t < ntargets; t++) {
        const uint32_t c0 = begin[t], c1 = end ? end[t] : begin[t + 1];
        if (c0 > c1 || c1 > nchunks) return -3;                             // a target's range outside the partials
    }
    const uint32_t W = B::AFF_W + 1;
    std::vector<uint32_t> part((size_t)nchunks * B::ACC_W * rows), cr((size_t)ntargets * B::ACC_W);
    for (uint32_t c = 0; c < nchunks; c++)
        for (uint32_t r = 0; r < rows; r++) {
            const uint32_t* w = partial + ((size_t)c * rows + r) * W;
            B::store(part.data(), c, r, rows, w, w[B::AFF_W] != 0, 2 + (c * 31 + r) % 97);      // the st_* layout of the gather kernels' partials
        }
    if (corr) for (uint32_t t = 0; t < ntargets; t++) B::store(cr.data(), t, 0, 1, corr + (size_t)t * W, corr[(size_t)t * W + B::AFF_W] != 0, 3 + t);
    DevBuf dpart, dbegin, dend, dcorr, dsums;
    const size_t swords = (size_t)ntargets * B::ACC_W * rows;
    hipError_t e = dpart.put(part.data(), part.size() * 4);
    if (e == hipSuccess) e = dbegin.put(begin, (size_t)(ntargets + 1) * 2);
    if (e == hipSuccess && end) e = dend.put(end, (size_t)ntargets * 2);
    if (e == hipSuccess && corr) e = dcorr.put(cr.data(), cr.size() * 4);
    if (e == hipSuccess) e = dsums.alloc(swords * 4);
    if (e == hipSuccess) e = hipMemset(dsums.p, 0xA5, swords * 4);
    if (e != hipSuccess) return (int)e;
    ReduceView R{};
    R.rows = rows; R.ntargets = ntargets; R.partial = dpart.as<uint32_t>(); R.target_chunk_begin = dbegin.as<uint16_t>();
    R.corr = corr ? dcorr.as<uint32_t>() : nullptr; R.target_chunk_end = end ? dend.as<uint16_t>() : nullptr;
    B::launch_sum(R, dsums.as<uint32_t>());
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    std::vector<uint32_t> sums(swords);
    if (e == hipSuccess) e = hipMemcpy(sums.data(), dsums.p, swords * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;
    for (uint32_t t = 0; t < ntargets; t++)
        for (uint32_t r = 0; r < rows; r++) B::words(out + ((size_t)t * rows + r) * W, sums.data(), t, r, rows);
    return 0;
}

}  // namespace

extern "C" {
// k_msm_gather through the product's launchers.  kind: 0 G1Msm, 1 G2Msm (g16_launch_msm), 2 EdGather, 3 EdGather in its raised-priority form
// (edg_launch_msm).  steps: [nsteps][2] as MsmView::steps; chunk_step0: [nchunks + 1]; digits: [digit_rows][rows] words of two int16
// digits; points / point_slot: npoints affine points and the table entry each is stored at, converted with the table builder's own
// per-entry code; table_entries: entries allocated (never cleared); acc_init: optional affine point; out: [nchunks][rows][17 | 33 | 17]
int devtier_msm(int kind, uint32_t rows, uint32_t nchunks, uint32_t nsteps, const uint32_t* steps, const uint32_t* chunk_step0, const uint32_t* digits, uint32_t digit_rows,
                const uint32_t* points, const uint64_t* point_slot, uint32_t npoints, uint64_t table_entries, const uint32_t* acc_init, uint32_t* out) {
    switch (kind) {
        case 0: return run_msm<BnG1>(false, rows, nchunks, nsteps, steps, chunk_step0, digits, digit_rows, points, point_slot, npoints, table_entries, acc_init, out);
        case 1: return run_msm<BnG2>(false, rows, nchunks, nsteps, steps, chunk_step0, digits, digit_rows, points, point_slot, npoints, table_entries, acc_init, out);
        case 2: case 3: return run_msm<Ed>(kind == 3, rows, nchunks, nsteps, steps, chunk_step0, digits, digit_rows, points, point_slot, npoints, table_entries, acc_init, out);
        default: return -1;
    }
}
// k_sum_t through g16_launch_sum (kind 0, 1: 32 slices per row) and edg_launch_sum (kind 2: 8 slices).  partial: [nchunks][rows][17 | 33 | 17]
// affine words + neutral flag, written in the st_* layout as projective representatives with Z != 1; begin: [ntargets + 1]; end: optional
// [ntargets]; corr: optional [ntargets][17 | 33 | 17]; out: [ntargets][rows][17 | 33 | 17]
int devtier_sum(int kind, uint32_t rows, uint32_t nchunks, uint32_t ntargets, const uint16_t* begin, const uint16_t* end, const uint32_t* partial, const uint32_t* corr, uint32_t* out) {
    switch (kind) {
        case 0: return run_sum<BnG1>(rows, nchunks, ntargets, begin, end, partial, corr, out);
        case 1: return run_sum<BnG2>(rows, nchunks, ntargets, begin, end, partial, corr, out);
        case 2: return run_sum<Ed>(rows, nchunks, ntargets, begin, end, partial, corr, out);
        default: return -1;
    }
}
int devtier_fe(int op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, int on_device) { return run_family<FeCase>(op, n, a, b, c, out, on_device); }
int devtier_fq(int op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, int on_device) { return run_family<FqCase>(op, n, a, b, c, out, on_device); }
int devtier_fq9(int op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, int on_device) { return run_family<Fq9Case>(op, n, a, b, c, out, on_device); }
int devtier_fr9(int op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, int on_device) { return run_family<Fr9Case>(op, n, a, b, c, out, on_device); }
int devtier_f128(int op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, int on_device) { return run_family<F128Case>(op, n, a, b, c, out, on_device); }
int devtier_sc(int op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, int on_device) { return run_family<ScCase>(op, n, a, b, c, out, on_device); }
int devtier_fp(int op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, int on_device) { return run_family<FpCase>(op, n, a, b, c, out, on_device); }
int devtier_ge(int op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, int on_device) { return run_family<GeCase>(op, n, a, b, c, out, on_device); }
int devtier_point(int op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, int on_device) { return run_family<PointCase>(op, n, a, b, c, out, on_device); }
}

// the Groth16 key tables, recodings and their join (entry points of their own)
#include "devtier_g16.h"
