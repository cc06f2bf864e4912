/* libzkp_hip -- the Groth16 key check: what a key file holds, and what the library built from it, tested on the GPU.
 *
 * zkp_hip_groth16_load_key applies what ark's deserialize_uncompressed (Validate::Yes) applies to a key file -- canonical words, points on
 * the curve, G2 points in the prime-order subgroup -- and self-checks the window tables it builds before it registers them
 * (ZKP_HIP_G16_TABLE_CHECK=0 skips that).  zkpkeycheck_key reports the same for a key blob without loading it, adds the
 * check ark does not make (a proving key's b_g1_query / b_g2_query, beta and delta twins share their discrete logarithms), and re-checks
 * the tables that are resident on the calling thread's shard.
 *
 * The stages, in the order they run; a stage that fails ends the check and names itself in `verdict`:
 *   POINTS  the format and the shape for the circuit `kind` (on the host), then one GPU lane per finite G2 point: r * Q is the identity
 *   TWINS   proving keys only.  The infinity flags of b_g1_query[i] and b_g2_query[i] must agree at every i.  Over the indices at which
 *           both are finite, with fresh 128-bit weights rho_i from the operating system, the GPU computes S1 = sum rho_i b_g1_query[i] and
 *           S2 = sum rho_i b_g2_query[i]; the host accepts iff e(S1, beta_g2) == e(beta_g1, S2) and e(beta_g1, delta_g2) == e(delta_g1,
 *           beta_g2).  A key that breaks the first identity is accepted with probability 2^-128.
 *   TABLES  every entry of every window table of the key loaded on this shard for `kind`, against the points of `key`: the two MSM tables
 *           of a proving key and the gamma_abc_g1 / alpha tables of the verifier.  `key` must be the blob that was loaded (SHA-256).
 *
 * The two functions of this header are zkpkeycheck_key and zkpkeycheck_counters -- one word before the underscore, because the zkp_* and
 * libzkp_* names of the library are closed sets that the ABI tests pin symbol by symbol; the constants and the report type keep the
 * ZKP_KEYCHECK_ / zkp_keycheck_ spelling.  include/libzkp_hip.h and its symbol set are unchanged.
 */
#ifndef LIBZKP_HIP_KEYCHECK_H
#define LIBZKP_HIP_KEYCHECK_H
#include "libzkp_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* `what`: the stages to run (POINTS always runs: the others read the parsed key) */
#define ZKP_KEYCHECK_POINTS 1u   /* format, shape, G2 subgroup membership: what the loader enforces */
#define ZKP_KEYCHECK_TWINS  2u   /* proving keys: the weighted pairing identities above */
#define ZKP_KEYCHECK_TABLES 4u   /* the tables resident on the calling thread's shard, against this key's points */

/* report.verdict: 0, or the first stage that failed */
#define ZKP_KEYCHECK_SOUND 0u
#define ZKP_KEYCHECK_FAILED_FORMAT 1u    /* malformed, or not a key of circuit `kind`: report.message holds the loader's message */
#define ZKP_KEYCHECK_FAILED_SUBGROUP 2u  /* a G2 point outside the prime-order subgroup */
#define ZKP_KEYCHECK_FAILED_TWINS 3u
#define ZKP_KEYCHECK_FAILED_TABLES 4u

/* report.format */
#define ZKP_KEYCHECK_FORMAT_PROVING_KEY 0u
#define ZKP_KEYCHECK_FORMAT_VERIFYING_KEY 1u
#define ZKP_KEYCHECK_FORMAT_UNKNOWN 2u   /* the blob could not be read as either */

/* report.table_first_which */
#define ZKP_KEYCHECK_TABLE_G1 0   /* the G1 MSM tables (a_query, b_g1_query, l_query, h_query, alpha, beta, delta: the loader's slots) */
#define ZKP_KEYCHECK_TABLE_G2 1   /* the G2 MSM tables (b_g2_query, delta, beta) */
#define ZKP_KEYCHECK_TABLE_VK 2   /* the verifier's tables: slot i < n is gamma_abc_g1[i], slot n is alpha_g1 */

typedef struct zkp_keycheck_report {
    uint32_t format;               /* ZKP_KEYCHECK_FORMAT_* */
    uint32_t verdict;              /* ZKP_KEYCHECK_SOUND or ZKP_KEYCHECK_FAILED_* */
    uint32_t stages_run;           /* mask of the ZKP_KEYCHECK_* stages that ran to their end */
    /* POINTS */
    uint32_t g2_checked;           /* finite G2 points tested (3 + the finite b_g2_query points of a proving key) */
    uint32_t g2_outside;           /* of those, outside the subgroup */
    int32_t g2_first_outside;      /* the first such point in file order: 0 beta_g2, 1 gamma_g2, 2 delta_g2, 3 + i b_g2_query[i]; -1 none */
    /* TWINS: the two verdicts are 1 true, 0 false, -1 not applicable (a verifying key) or not run */
    uint32_t twins_checked;        /* indices at which b_g1_query[i] and b_g2_query[i] are both finite */
    uint32_t twin_inf_mismatches;  /* indices at which exactly one of the two is the point at infinity */
    int32_t twins_query_ok;        /* e(S1, beta_g2) == e(beta_g1, S2) */
    int32_t twins_beta_delta_ok;   /* e(beta_g1, delta_g2) == e(delta_g1, beta_g2) */
    /* TABLES */
    int32_t table_first_which;     /* ZKP_KEYCHECK_TABLE_* of the first bad entry; -1 none */
    uint32_t table_first_slot, table_first_window, table_first_entry;      /* a broken join of two windows is reported at entry 0 of the upper one */
    uint32_t table_bad_pairs;      /* (slot, window) pairs with an inconsistent entry, over all tables checked */
    uint64_t table_entries_g1, table_entries_g2, table_entries_vk;         /* entries checked per table */
    /* milliseconds per stage (host time around the stage, its device work included) */
    double ms_points, ms_twins, ms_tables;
    char message[160];             /* what failed, in words; empty when sound */
} zkp_keycheck_report;

/* Checks `key` (either format zkp_hip_groth16_load_key accepts) as a key of circuit `kind` (0 equality, 1 membership, as for the loader) on the
 * calling thread's shard, which is initialised on first use.  POINTS and TWINS need no loaded key.  TABLES needs `key` to be the key
 * loaded on this shard for `kind` (ZKP_HIP_E_ARGUMENT otherwise) and re-derives the slots under the same ZKP_HIP_G16_SHARE_AB.
 * Returns 0 when the check ran -- the verdict is in *report -- and a negative code for an argument or runtime error. */
int zkpkeycheck_key(int kind, const uint8_t* key, uint64_t len, uint32_t what, zkp_keycheck_report* report);

/* Summed over the shards, always counted: host milliseconds spent in table checks (at load and in zkpkeycheck_key), key loads whose
 * freshly built tables were checked, table entries checked, and keys refused (by the subgroup test or the table self-check at load, or by a
 * zkpkeycheck_key verdict other than SOUND).  Any pointer may be null; reset != 0 clears the counters. */
int zkpkeycheck_counters(double* ms, uint64_t* loads_checked, uint64_t* entries_checked, uint64_t* refused, int reset);

#ifdef __cplusplus
}
#endif
#endif
