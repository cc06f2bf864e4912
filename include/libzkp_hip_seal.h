/* libzkp_hip -- one call that seals a list of composite proofs.
 *
 * A composite proof ("COMP" container, CompositeProof of utils/composition.rs; libzkp_hip_composites.h is the verifier's half) holds 1 to
 * 1000 envelopes, optional metadata, and a SHA-256 digest over both.  The calls of this header make n of them at once: the sizes, offsets
 * and statuses of all containers come from one host pass over the envelopes' lengths and header bytes and the metadata (before any device
 * work), the containers are framed on the GPU, one wave per inner proof or metadata run, and the digests are computed on the GPU, one
 * container per lane.  libzkp_seal_batch does it for a proved staged batch without the proofs crossing to the host first.
 *
 * The bytes are those of the reference's create_composite_proof / create_proof_with_metadata (advanced/composite.rs:10-59) with the
 * metadata entries written in the order the caller gives them (the reference iterates a HashMap there: any order is a valid encoding; the
 * digest does not depend on it).
 *
 * Both sealing calls run on one shard: libzkp_seal_composites on the calling thread's (zkp_hip_use_device), libzkp_seal_batch on the shard
 * that holds the batch, or -- for a batch staged on several shards -- on the calling thread's.  A call is not spread over the registered
 * shards.
 *
 * A digest is computed by one lane, whatever the container's size: one 4 MiB container is the worst case of these calls, as it is of
 * zkp_hip_verify_composites.
 *
 * The symbols of this header begin with libzkp_seal_, not zkp_: the zkp_* names of the library are a closed set.
 */
#ifndef LIBZKP_HIP_SEAL_H
#define LIBZKP_HIP_SEAL_H
#include "libzkp_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* status[i] of container i */
#define LIBZKP_SEAL_FAILED_OP 0u  /* libzkp_seal_batch only: one of its ops has a status other than 0 (it failed validation, or a flagged
                                     self-check refused its proof) */
#define LIBZKP_SEAL_SEALED 1u     /* the container was written */
#define LIBZKP_SEAL_REFUSED 2u    /* the reference's own creation returns Err: the proof list is empty, or Proof::from_bytes refuses an
                                     envelope (shorter than 10 bytes, longer than 1 MiB, a payload above 900 KiB, a commitment above 256
                                     bytes, or a length that is not 10 + payload + commitment) */
#define LIBZKP_SEAL_UNREADABLE 3u /* THIS LIBRARY'S RULE, not upstream's: the reference would write the container, but
                                     CompositeProof::from_bytes would refuse to read it back -- more than 1000 proofs or metadata entries, a
                                     key longer than 1024 bytes or that String::from_utf8 refuses, a value longer than 65536 bytes, a
                                     metadata run that is truncated or has bytes left over, a container longer than 4 MiB -- or a key
                                     occurs twice (upstream takes a HashMap; a repeated key has no single meaning here) */

/* Host buffers.  Envelope e is env_blob[env_off[e] .. env_off[e + 1]) (env_off: n_env + 1 entries), as for zkp_hip_verify_envelopes.
 * Container i takes the envelopes first[i] .. first[i + 1] (first: n + 1 entries that do not decrease and stay within [0, n_env]) and the
 * metadata meta_blob[meta_off[i] .. meta_off[i + 1]), already in wire form, (u32 key_len | key | u32 value_len | value)*, written to the
 * container in exactly that order; meta_blob and meta_off may both be NULL: no container has metadata.
 * Container i is written to out[out_off[i] .. out_off[i + 1]) (out_off: n + 1 entries); a container that is not sealed takes zero bytes,
 * so out_off is a compact prefix sum.  status: n bytes.
 * Returns 0, or 1 when some container was not sealed, or a negative code with a message (zkp_hip_last_error).  When out_cap is too small
 * the call returns ZKP_HIP_E_ARGUMENT, out_off[n] holds the size needed, and nothing is written to out.  n = 0 returns 0 and touches
 * nothing.  More than 2^22 containers or envelopes, a null pointer, or a `first` or meta_off that decreases or leaves its range, is
 * ZKP_HIP_E_ARGUMENT, before any device work. */
int libzkp_seal_composites(uint64_t n,
                           const uint8_t* env_blob, const uint64_t* env_off, uint64_t n_env,
                           const uint64_t* first,
                           const uint8_t* meta_blob, const uint64_t* meta_off,
                           uint8_t* out, uint64_t out_cap, uint64_t* out_off, uint8_t* status);

/* The same for a staged batch (zkp_hip_batch_stage) that has been launched; the call waits for it by itself, as zkp_hip_batch_fetch does.
 * Container i holds the proofs of the ops first_op[i] .. first_op[i + 1] in the caller's op order; every proof of an op with status 0
 * counts as accepted (it is the library's own output).  A container with an op whose status is not 0 gets LIBZKP_SEAL_FAILED_OP and zero
 * bytes.  For a batch staged on one shard the containers are framed and hashed from the packed proofs where they lie in device memory: no
 * envelope byte crosses to the host before the sealed containers do.  A batch staged on several shards has one container's ops on several
 * GPUs: the call then fetches the proofs once into a scratch buffer, as zkp_hip_batch_fetch does, and takes the host-buffer path.
 * The batch is neither freed nor changed: zkp_hip_batch_fetch afterwards returns what it always returned. */
int libzkp_seal_batch(zkp_hip_batch* batch, uint64_t n, const uint64_t* first_op,
                      const uint8_t* meta_blob, const uint64_t* meta_off,
                      uint8_t* out, uint64_t out_cap, uint64_t* out_off, uint8_t* status);

/* Always counted, per shard, summed over the shards: *ms = host wall time of the device half of the calls, *containers = containers
 * seen, *sealed = containers given status 1, *envelopes = inner proofs of the sealed containers, *bytes = bytes of the sealed containers.
 * A call that fails its argument checks, or whose out_cap is too small, counts nothing.  Any pointer may be NULL. */
int libzkp_seal_counters(double* ms, uint64_t* containers, uint64_t* sealed,
                         uint64_t* envelopes, uint64_t* bytes, int reset);

#ifdef __cplusplus
}
#endif
#endif
