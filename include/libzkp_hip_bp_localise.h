/* libzkp_hip -- the Bulletproofs verifiers after a batch check that did not stand.
 *
 * From ZKP_HIP_BATCH_VERIFY_MIN jobs up, zkp_hip_verify_range_batch / _threshold_batch / _consistency_batch (libzkp_hip.h) and everything
 * built on them -- the mixed verifier (libzkp_hip_verify.h), the self-check of a staged batch, a call spread over several GPUs, per slice --
 * check the whole batch with one random linear combination.  When that check does not stand, the call no longer verifies every job again:
 * the batch is cut into contiguous segments of envelopes, every segment gets the same check over its own jobs from what the failed check
 * left in device memory (nothing is decoded, replayed or drawn again), and only the jobs of the suspect segments go through the per-job
 * pass.  When the suspect segments hold half of the batch's jobs or more, the whole batch is verified job by job as before.  The verdicts
 * are those of the per-job pass; envelopes refused by a parse or decode rule never enter a sum and make no segment suspect.
 *
 * Soundness: a segment's check uses only its own jobs' weights (independent 128-bit draws), so a call or slice errs with probability at
 * most (1 + segments) * 2^-128.
 *
 * Switches, read on every call:
 *   ZKP_HIP_BP_LOCALISE=0                     no segment checks: the per-job pass over the whole batch
 *   ZKP_HIP_BP_LOCALISE_SEGMENT=<envelopes>   segment size (default: about n / 256, a multiple of 16 and at least 32; raised until there are
 *                                             at most 1024 segments)
 *   ZKP_HIP_BP_BATCH_VERIFY_ONLY              as before: the call fails at the batch check, before any localisation
 */
#ifndef LIBZKP_HIP_BP_LOCALISE_H
#define LIBZKP_HIP_BP_LOCALISE_H
#include "libzkp_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* What the Bulletproofs verifiers did after batch checks that did not stand; always counted, per shard, summed over the shards.
 * *failed_checks = batch checks (calls or slices) that did not stand; *segment_checks = segments checked;
 * *jobs_again = jobs given the per-job pass after a failed check (the compacted suspects, or M when the whole batch was verified again);
 * *ms = host wall time from the failed check's verdict to the call's return.  Any pointer may be NULL. */
int zkp_hip_bp_localise_counters(double* ms, uint64_t* failed_checks, uint64_t* segment_checks, uint64_t* jobs_again, int reset);

#ifdef __cplusplus
}
#endif
#endif
