// TEST INFRASTRUCTURE, not part of libzkp_hip.so: the device tier of the Groth16 verifier's arithmetic (bn254_g.h's Fq2, bn254_pairing.h,
// fq2vm.h, fq2vm_programs.h).  Operands and results are RAW LIMBS, as in devtier.hip, whose runner it shares (devtier_family.h).
//   devtier_fq2      one Fq2 operation per case through the machine's own ALU switch (fq2vm::alu), ids = fq2vm::Op values
//   devtier_fq12     the lane-per-chain tower: Fq6 / Fq12 arithmetic, the line functions, the Miller loop, the final exponentiations
//   devtier_fq2vm    one chain of the Fq2 machine over a caller-filled slot buffer: fq2vm::run_host per envelope, or ONE launch of the
//                    product's own k_fq2vm through g16_vm_launch_chain / g16_vm_launch_script of libzkp_hip.so
// Cases and bigint references: tests/devtier_pairing_cases.py.
#include "../../libzkp_amd/csrc/fq2vm.h"
#include "../../libzkp_amd/csrc/g16_verify_launch.h"
#include "devtier_family.h"
#include <cstring>
#include <vector>
using namespace zkp;
using namespace devtier;

namespace {

ZKP_HD inline fq2 ld2(const uint32_t* w) { return fq2{ld<fq, 10>(w), ld<fq, 10>(w + 10)}; }
ZKP_HD inline void st2(uint32_t* w, const fq2& x) { st<fq, 10>(w, x.c0); st<fq, 10>(w + 10, x.c1); }
ZKP_HD inline void raw2(uint32_t* w, const fq2& x) { fq_to_raw(w, x.c0); fq_to_raw(w + 8, x.c1); }

// ------------------------------------------------------------------------------------------------ fq2: the machine's ALU
// a, b: 20 raw limbs (c0 then c1).  result: 20 raw limbs, 16 canonical words (fq_to_raw of each component), 1 flag
constexpr int FQ2_DBL = 32, FQ2_IS_ZERO = 33, FQ2_EQ = 34;
struct Fq2Case {
    ZKP_HD static Shape shape(int op) {
        switch (op) {
            case fq2vm::MUL: case fq2vm::ADD: case fq2vm::SUB: case fq2vm::MUL0: case fq2vm::MUL1: case fq2vm::T3M: case fq2vm::T3P: case FQ2_EQ: return Shape{20, 20, 0, 37};
            case fq2vm::SQ: case fq2vm::MULXI: case fq2vm::CONJ: case fq2vm::INV: case fq2vm::NEG: case fq2vm::MOV: case FQ2_DBL: case FQ2_IS_ZERO: return Shape{20, 0, 0, 37};
            default: return Shape{0, 0, 0, 0};
        }
    }
    ZKP_HD static void run(int op, const uint32_t* a, const uint32_t* b, const uint32_t*, uint32_t* out) {
        const fq2 x = ld2(a);
        fq2 r = x; uint32_t flag = 0;
        if (op == FQ2_DBL) r = f_dbl(x);
        else if (op == FQ2_IS_ZERO) flag = f_is_zero(x) ? 1u : 0u;
        else if (op == FQ2_EQ) flag = fq2_eq(x, ld2(b)) ? 1u : 0u;
        else r = fq2vm::alu((uint32_t)op, x, fq2vm::op_has_b((uint32_t)op) ? ld2(b) : x);
        st2(out, r);
        raw2(out + 20, r);
        out[36] = flag;
    }
};

// ------------------------------------------------------------------------------------------------ fq12: the lane-per-chain tower
// An Fq12 element is 12 x 10 raw limbs in tower order (c0.a0.c0, c0.a0.c1, c0.a1.c0, ... c1.a2.c1).  result: 120 raw limbs, 96 canonical words,
// 1 flag; an Fq6 result is c0 of it, a line's three coefficients A, B, C its first three Fq2 (the rest zero)
enum { F6_MUL, F6_INV, F12_MUL, F12_SQ, F12_MUL_LINE, F12_INV, F12_CONJ, F12_FROB2, F12_FROB1, F12_FROB3, F12_CYCLO_SQ, F12_POW_X, F12_IS_ONE, LINE_DOUBLE, LINE_ADD,
       MILLER, FINAL_EXP, FINAL_EXP_CHAIN };
constexpr uint32_t F12_OUT = 120 + 96 + 1;
ZKP_HD inline fq6 ld6(const uint32_t* w) { return fq6{ld2(w), ld2(w + 20), ld2(w + 40)}; }
ZKP_HD inline fq12 ld12(const uint32_t* w) { return fq12{ld6(w), ld6(w + 60)}; }
struct Fq12Case {
    ZKP_HD static Shape shape(int op) {
        switch (op) {
            case F6_MUL: return Shape{60, 60, 0, F12_OUT};
            case F6_INV: return Shape{60, 0, 0, F12_OUT};
            case F12_MUL: return Shape{120, 120, 0, F12_OUT};
            case F12_MUL_LINE: return Shape{120, 60, 0, F12_OUT};
            case F12_SQ: case F12_INV: case F12_CONJ: case F12_FROB2: case F12_FROB1: case F12_FROB3: case F12_CYCLO_SQ: case F12_POW_X: case F12_IS_ONE:
            case FINAL_EXP: case FINAL_EXP_CHAIN: return Shape{120, 0, 0, F12_OUT};
            case LINE_DOUBLE: return Shape{60, 20, 0, F12_OUT};          // T (X, Y, Z); (xp, yp)
            case LINE_ADD: return Shape{60, 60, 0, F12_OUT};             // T; Q (x, y), (xp, yp)
            case MILLER: return Shape{40, 20, 0, F12_OUT};               // Q (x, y); P (x, y)
            default: return Shape{0, 0, 0, 0};
        }
    }
    ZKP_HD static void put(uint32_t* out, const fq12& r, uint32_t flag) {
        const fq2* k[6] = {&r.c0.a0, &r.c0.a1, &r.c0.a2, &r.c1.a0, &r.c1.a1, &r.c1.a2};
        for (int i = 0; i < 6; i++) { st2(out + 20 * i, *k[i]); raw2(out + 120 + 16 * i, *k[i]); }
        out[216] = flag;
    }
    ZKP_HD static void run(int op, const uint32_t* a, const uint32_t* b, const uint32_t*, uint32_t* out) {
        fq12 r = fq12{fq6_zero(), fq6_zero()};
        uint32_t flag = 0;
        switch (op) {
            case F6_MUL: r.c0 = fq6_mul(ld6(a), ld6(b)); break;
            case F6_INV: r.c0 = fq6_inv(ld6(a)); break;
            case F12_MUL: r = fq12_mul(ld12(a), ld12(b)); break;
            case F12_SQ: r = fq12_sq(ld12(a)); break;
            case F12_MUL_LINE: r = fq12_mul_line(ld12(a), fq12_line{ld2(b), ld2(b + 20), ld2(b + 40)}); break;
            case F12_INV: r = fq12_inv(ld12(a)); break;
            case F12_CONJ: r = fq12_conj(ld12(a)); break;
            case F12_FROB2: r = fq12_frob_p2(ld12(a)); break;
            case F12_FROB1: r = fq12_frob_odd(ld12(a), 1); break;
            case F12_FROB3: r = fq12_frob_odd(ld12(a), 3); break;
            case F12_CYCLO_SQ: r = fq12_cyclo_sq(ld12(a)); break;
            case F12_POW_X: r = fq12_pow_x(ld12(a)); break;
            case F12_IS_ONE: r = ld12(a); flag = fq12_is_one(r) ? 1u : 0u; break;
            case LINE_DOUBLE: case LINE_ADD: {
                const g2_jac T{ld2(a), ld2(a + 20), ld2(a + 40)};
                const fq2 p = ld2(op == LINE_DOUBLE ? b : b + 40);
                const fq12_line l = op == LINE_DOUBLE ? line_double(T, p.c0, p.c1) : line_add(T, g2_aff{ld2(b), ld2(b + 20)}, p.c0, p.c1);
                r.c0 = fq6{l.A, l.B, l.C};
                break;
            }
            case MILLER: { const fq2 p = ld2(b); r = miller_loop(g2_aff{ld2(a), ld2(a + 20)}, g1_aff{p.c0, p.c1}); break; }
            case FINAL_EXP: r = final_exponentiation(ld12(a)); break;
            default: r = final_exponentiation_chain(ld12(a)); break;
        }
        put(out, r, flag);
    }
};

// ------------------------------------------------------------------------------------------------ the Fq2 machine, chain by chain
namespace vm = fq2vm;
constexpr uint32_t VM_GUARD = 4096, VM_FILL = 0xA5A5A5A5u, VM_MAX_N = 4096;
struct Chain { const uint16_t* script; uint32_t len, nregs, slots, kwords; };
// 0 = A, 1 = subgroup, 2 = finish, 3 = B (as G16VmTables::script), 4 = lines.  slots: the slot buffer a launch may touch; kwords: its constant table
Chain chain_of(int c) {
    switch (c) {
        case 0: return Chain{vm::SCRIPT_MILLER, (uint32_t)(sizeof(vm::SCRIPT_MILLER) / 2), vm::REGS_K4[0], vm::N_SLOTS, 0};
        case 1: return Chain{vm::SCRIPT_SUBGROUP, (uint32_t)(sizeof(vm::SCRIPT_SUBGROUP) / 2), vm::REGS_K4[1], vm::N_SLOTS, 0};
        case 2: return Chain{vm::SCRIPT_FINISH, (uint32_t)(sizeof(vm::SCRIPT_FINISH) / 2), vm::REGS_K4[2], vm::N_SLOTS, 6 * vm::FQ2_W};
        case 3: return Chain{vm::SCRIPT_MILLER_B, (uint32_t)(sizeof(vm::SCRIPT_MILLER_B) / 2), vm::REGS_K4[3], vm::N_SLOTS, (uint32_t)vm::N_LINE_SLOTS * vm::FQ2_W};
        case 4: return Chain{vm::SCRIPT_LINES, (uint32_t)(sizeof(vm::SCRIPT_LINES) / 2), vm::REGS_K4[4], (uint32_t)(vm::LINE_SLOT0 + vm::N_LINE_SLOTS), 0};
        default: return Chain{nullptr, 0, 0, 0, 0};
    }
}
// Nothing is launched unless every register, slot and constant a chain's micro-operations name is inside what this library allocates: the
// walk below follows the tables exactly as the interpreter does (per wave, from the script entry's offset to END, the cursor advancing).
bool chain_in_bounds(const Chain& c) {
    const uint32_t K = 4, ncode = (uint32_t)(sizeof(vm::CODE_K4) / 4);
    uint32_t cur = 0;
    for (uint32_t s = 0; s < c.len; cur += c.script[s] >> 8, s++) {
        const uint32_t prog = c.script[s] & 255u;
        if (prog >= vm::N_PROGRAMS) return false;
        for (uint32_t w = 0; w < K; w++) {
            for (uint32_t pc = vm::OFF_K4[prog * K + w];; pc += 2) {
                if (pc + 1 >= ncode) return false;
                const uint32_t u0 = vm::CODE_K4[pc], u1 = vm::CODE_K4[pc + 1], op = u0 & 0x7fu;
                if (op == vm::END) break;
                if (op > vm::END) return false;
                for (int h = 0; h < 2; h++) {
                    if (h == 1 && !(u1 & 1u)) continue;
                    const uint32_t t = h ? u1 : u0, d = (t >> 8) & 255u, a = (t >> 16) & 255u, b = t >> 24;
                    const bool imm = op == vm::LDG || op == vm::LDC || op == vm::LDK || op == vm::STG || op == vm::STC;
                    if (op != vm::NOP && op != vm::STG && op != vm::STC && d >= c.nregs) return false;
                    if (op != vm::NOP && op != vm::LDG && op != vm::LDC && op != vm::LDK && a >= c.nregs) return false;
                    if (!imm && vm::op_has_b(op) && b >= c.nregs) return false;
                    if ((op == vm::LDG || op == vm::STG) && b >= c.slots) return false;
                    if (op == vm::STC && cur + b >= c.slots) return false;
                    if (op == vm::LDC && b >= vm::N_CONSTS) return false;
                    if (op == vm::LDK && (size_t)(cur + b + 1) * vm::FQ2_W > c.kwords) return false;
                }
            }
        }
    }
    return c.nregs * vm::FQ2_W * vm::G * 4 <= 160u * 1024u;
}

G16VmTables g_tables;
const uint16_t* g_lines_script = nullptr;
int tables_ready() {
    if (!g_tables.ready && g16_vm_upload(g_tables) != 0) return -2;
    if (!g_lines_script) {
        void* p = nullptr;
        if (hipMalloc(&p, sizeof(vm::SCRIPT_LINES)) != hipSuccess) return -2;
        if (hipMemcpy(p, vm::SCRIPT_LINES, sizeof(vm::SCRIPT_LINES), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(p); return -2; }
        g_lines_script = static_cast<const uint16_t*>(p);
    }
    return 0;
}

}  // namespace

extern "C" {

int devtier_fq2(int op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, int on_device) { return run_family<Fq2Case>(op, n, a, b, c, out, on_device); }
int devtier_fq12(int op, uint32_t n, const uint32_t* a, const uint32_t* b, const uint32_t* c, uint32_t* out, int on_device) { return run_family<Fq12Case>(op, n, a, b, c, out, on_device); }

// slots of a chain's buffer and words of its constant table: out = {slots, kconst words, registers, script entries}
int devtier_fq2vm_geom(int chain, uint32_t* out) {
    const Chain c = chain_of(chain);
    if (!c.script || !out) return -1;
    out[0] = c.slots; out[1] = c.kwords; out[2] = c.nregs; out[3] = c.len;
    return 0;
}
// io: [slots][20][n], filled by the caller, comes back as the chain leaves it.  -7: a word of the guards around the device buffer changed
int devtier_fq2vm(int chain, uint32_t n, uint32_t* io, const uint32_t* kconst, int on_device) {
    const Chain c = chain_of(chain);
    if (!c.script || !io || !n || n > VM_MAX_N || (c.kwords && !kconst)) return -1;
    if (!chain_in_bounds(c)) return -8;
    const size_t words = (size_t)c.slots * vm::FQ2_W * n;
    if (!on_device) {
        const vm::Tables T{vm::CODE_K4, vm::OFF_K4, 4, &vm::CONSTS[0][0]};
        const vm::Launch L{T, c.script, c.len, n, io, 0, kconst};
        for (uint32_t i = 0; i < n; i++) vm::run_host(L, i, c.nregs);
        return 0;
    }
    if (tables_ready() != 0) return -2;
    std::vector<uint32_t> h(words + 2 * VM_GUARD, VM_FILL);
    memcpy(h.data() + VM_GUARD, io, words * 4);
    uint32_t *d_io = nullptr, *d_k = nullptr;
    hipError_t e = hipMalloc((void**)&d_io, h.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(d_io, h.data(), h.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && c.kwords) {
        e = hipMalloc((void**)&d_k, (size_t)c.kwords * 4);
        if (e == hipSuccess) e = hipMemcpy(d_k, kconst, (size_t)c.kwords * 4, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) {
        if (chain < 4) g16_vm_launch_chain(g_tables, chain, n, d_io + VM_GUARD, d_k, nullptr);
        else g16_vm_launch_script(g_tables, g_lines_script, c.len, c.nregs, n, d_io + VM_GUARD, d_k, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h.data(), d_io, h.size() * 4, hipMemcpyDeviceToHost);
    if (d_io) (void)hipFree(d_io);
    if (d_k) (void)hipFree(d_k);
    if (e != hipSuccess) return (int)e;
    memcpy(io, h.data() + VM_GUARD, words * 4);
    for (size_t i = 0; i < VM_GUARD; i++) if (h[i] != VM_FILL || h[VM_GUARD + words + i] != VM_FILL) return -7;
    return 0;
}

}  // extern "C"
