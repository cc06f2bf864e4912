// Host-callable launchers of the Groth16 verification kernels (g16_verify_kernels.hip: one lane per chain; fq2vm_kernels.hip: the
// Fq2 virtual machine, K waves per chain).
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "g16_verify.h"
#include "g16_localise.h"

size_t g16_verify_scratch_bytes(uint32_t n);     // device scratch for n envelopes (Miller-loop values, parsed points)
void g16_launch_verify(int kind, const uint8_t* d_in, uint64_t stride, const uint32_t* d_len, uint32_t n, const zkp::G16Vk& vk, void* d_scratch, uint8_t* d_ok, hipStream_t st);

// ---- Fq2 virtual machine (fq2vm.h): micro-operation tables in device memory, one set per device
struct G16VmTables {
    const uint32_t *code = nullptr, *off = nullptr;                                 // four waves per chain (fq2vm_programs.h)
    const uint32_t* consts = nullptr;
    const uint16_t* script[4] = {nullptr, nullptr, nullptr, nullptr};               // chain A, subgroup, finish, chain B
    hipStream_t side[2] = {nullptr, nullptr}; hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // chain B and the subgroup chain run beside chain A
    hipStream_t vq[2] = {nullptr, nullptr};        // the batch check's virtual envelope: greatest priority, so that its one-workgroup chains get the first CU that drains
    hipStream_t sub = nullptr, tail = nullptr;      // the batch check of several rounds: its subgroup chain on every CU but the first of each XCD, the one-workgroup tail (product, finishing chain) on those eight
    bool ready = false;
};
int g16_vm_upload(G16VmTables& T);
void g16_vm_free(G16VmTables& T);
// One launch of the machine on the slot buffer io[slot][20][count].  chain: 0 = A, 1 = subgroup, 2 = finish, 3 = B (its script in T.script, its
// length and register count from fq2vm_programs.h); the explicit form takes any script in device memory with its register count (chain L).
void g16_vm_launch_chain(const G16VmTables& T, int chain, uint32_t count, uint32_t* io, const uint32_t* kconst, hipStream_t s);
void g16_vm_launch_script(const G16VmTables& T, const uint16_t* script, uint32_t script_len, uint32_t nregs, uint32_t count, uint32_t* io, const uint32_t* kconst, hipStream_t s);
// per key: the machine's Miller value of (beta, -alpha) and the line table of gamma and delta (host computation through the same tables)
void g16_vm_key_constants(const zkp::g2_aff& beta, const zkp::g1_aff& neg_alpha, const zkp::g2_aff& gamma, const zkp::g2_aff& delta, uint32_t ml[6 * 20], std::vector<uint32_t>& lines);
size_t g16_vm_scratch_bytes(uint32_t n);
// verdicts of the generic envelopes in d_ok (0 for the others); *d_special (zeroed by the caller) counts the envelopes with a point at infinity in
// the proof, whose verdicts only g16_launch_verify gives
void g16_launch_verify_vm(int kind, const uint8_t* d_in, uint64_t stride, const uint32_t* d_len, uint32_t n, const zkp::G16Vk& vk, const G16VmTables& T, const uint32_t* d_kconst,
                          const uint32_t* d_lines, void* d_scratch, uint8_t* d_ok, uint32_t* d_special, hipStream_t st);
// One pairing check for the whole batch (g16_rlc.h).  d_scratch: g16_rlc_scratch_bytes(n, vk.n_ic) bytes with the weights (4 words per envelope,
// non-zero) at g16_rlc_rho_offset and four zeroed counters at g16_rlc_counters_offset: [0] envelopes with a point at infinity, [1] live envelopes
// whose B is outside the subgroup, [2] anomalies of the virtual envelope, [3] 1 when the batch's product is one.  d_ok holds the verdicts when
// counters == {0, 0, 0, 1}; otherwise the caller verifies envelope by envelope.
size_t g16_rlc_scratch_bytes(uint32_t n, uint32_t n_ic);
size_t g16_rlc_rho_offset(uint32_t n, uint32_t n_ic);
size_t g16_rlc_counters_offset(uint32_t n, uint32_t n_ic);
void g16_launch_verify_rlc(int kind, const uint8_t* d_in, uint64_t stride, const uint32_t* d_len, uint32_t n, const zkp::G16Vk& vk, const G16VmTables& T, const uint32_t* d_kconst,
                           const uint32_t* d_lines, void* d_scratch, uint8_t* d_ok, hipStream_t st);
// Which envelopes are bad, after a batch check that did not stand (g16_localise.h): one virtual envelope per segment from what the check left in
// d_rlc (its scratch, complete) and d_ok (its verdicts); leaves one suspect byte per segment at the start of d_loc (g16_loc_scratch_bytes(g.count,
// vk.n_ic) bytes).  The caller turns those into offsets (g16_loc_offsets, to g16_loc_offsets_offset of d_loc), compacts the suspect segments'
// envelopes, verifies them and scatters their verdicts back over d_ok.
size_t g16_loc_scratch_bytes(uint32_t nseg, uint32_t n_ic);
size_t g16_loc_offsets_offset(uint32_t nseg, uint32_t n_ic);
void g16_launch_localise(int kind, const uint8_t* d_in, uint64_t stride, const uint32_t* d_len, uint32_t n, const zkp::G16Segments& g, const zkp::G16Vk& vk, const G16VmTables& T,
                         const uint32_t* d_kconst, const uint32_t* d_lines, void* d_rlc, const uint8_t* d_ok, void* d_loc, hipStream_t st);
void g16_launch_compact(const uint8_t* d_in, uint64_t stride, const uint32_t* d_len, uint32_t n, const zkp::G16Segments& g, const uint8_t* d_suspect, const uint32_t* d_off,
                        uint8_t* d_in2, uint32_t* d_len2, hipStream_t st);
void g16_launch_scatter(uint32_t n, const zkp::G16Segments& g, const uint8_t* d_suspect, const uint32_t* d_off, const uint8_t* d_ok2, uint8_t* d_ok, hipStream_t st);
