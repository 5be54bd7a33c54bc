/*
 * lo_iris_batch.h — C ABI of the batched LiDAR-Iris detector: B independent descriptor databases, one per job of an
 * lo_batch (lo_icp.h), behind one handle.  The keyframes of any subset of jobs are added, and the queries of any
 * subset of jobs are answered, in a fixed number of stream operations and one synchronise, whatever the subset's size
 * (DESIGN.md "Batched detector").
 *
 * Per job everything is the solo detector's (lo_iris.h), bit for bit: the same image, encode and per-shift match
 * arithmetic (the kernels share their device bodies), the same NaN and tie rules, the same selection rule.  The one
 * difference is the order of work in lo_iris_batch_detect: the two tests of lo_iris_select_host that need no distance
 * (keyframe gap, position norm) are applied on the host BEFORE the match, and only the (query, entry) pairs that pass
 * are matched.  An entry that fails either test can never be selected by the solo rule, so the candidate is the solo
 * detector's, field for field.
 *
 * Conventions as lo_iris.h.  The handle is created against a batch and uses that batch's device, stream and contexts;
 * the batch must outlive it.  Every call is synchronous, runs on the batch stream, needs the contexts idle (as every
 * batch call) and returns LO_ERR_STATE while the batch has an optimize in flight.  Not thread-safe.  Not wired into
 * lo_odom_batch_* yet (lo_odometry.h).
 *
 * Job lists: `jobs` holds k distinct job indices in [0, lo_batch_size); a duplicate or an out-of-range index gives
 * LO_ERR_ARG and nothing is enqueued.  Per-job arrays (ids, positions (3 per job), pts, n, status, cand) are indexed
 * by the position in the list, not by the job index.
 */
#ifndef LO_IRIS_BATCH_H
#define LO_IRIS_BATCH_H

#include <stddef.h>
#include <stdint.h>

#include "lo_iris.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lo_iris_batch lo_iris_batch;

/* capacity_per_job: database entries per job, fixed; 43,200 B of device memory each, for every job of the batch. */
lo_iris_batch* lo_iris_batch_create(lo_batch* b, size_t capacity_per_job, int* err);
void           lo_iris_batch_destroy(lo_iris_batch* ib);
const char*    lo_iris_batch_last_error(const lo_iris_batch* ib);
size_t         lo_iris_batch_size(const lo_iris_batch* ib, int job);
size_t         lo_iris_batch_capacity(const lo_iris_batch* ib);      /* per job */
int            lo_iris_batch_clear(lo_iris_batch* ib, int job);      /* job = -1: all */

/* lo_iris_add_keyframe for each listed job: its descriptor goes to slot size(job) of its database, its id and position
 * are pushed on the host.  pts[i]: host pointers, or (on_device != 0) device pointers on the batch's device.
 * status[i]: LO_OK, LO_INSUFFICIENT for an empty cloud (nothing added) or LO_ERR_CAPACITY for a full database
 * (nothing added for that job).  Returns the first negative per-job status after the other jobs are done, else
 * LO_OK; a whole-call error (LO_ERR_ARG, LO_ERR_STATE, LO_ERR_HIP) leaves status untouched. */
int lo_iris_batch_add(lo_iris_batch* ib, const int* jobs, int k, const int64_t* ids, const float* positions,
                      const float* const* pts_xyz, const size_t* n, int on_device, int* status);
/* lo_iris_add_from_scan for each listed job: the job's context's device-filtered scan (lo_batch_filter_raw*), read in
 * place.  The counts are the host's where it already knows them (after lo_batch_filter_raw* it does); otherwise one
 * readback fetches the counts of all k jobs.  status[i] also: LO_ERR_STATE for a context without such a scan. */
int lo_iris_batch_add_from_scans(lo_iris_batch* ib, const int* jobs, int k, const int64_t* ids,
                                 const float* positions, int* status);

/* lo_iris_detect for each listed job on its own database.  pts_xyz = NULL: the jobs' device-filtered scans (n and
 * on_device are then ignored).  status[i]: LO_OK with cand[i] filled, or LO_INSUFFICIENT (cand[i] untouched) for an
 * empty cloud, an empty database, no eligible entry or nothing under the threshold.  The current keyframes are not
 * added.  A job without an eligible entry costs no device work; if no job has one, nothing is launched. */
int lo_iris_batch_detect(lo_iris_batch* ib, const lo_iris_config* cfg, const int* jobs, int k, const int64_t* ids,
                         const float* positions, const float* const* pts_xyz, const size_t* n, int on_device,
                         lo_iris_candidate* cand, int* status);

/* Parity entry, ungated: lo_iris_compare_all for each listed job.  Job i's records are at [offsets[i], offsets[i+1])
 * of the output arrays, in insertion order; an empty query cloud gives that job zero records.  cap: the length of the
 * output arrays; LO_ERR_CAPACITY (nothing written but offsets) if the records do not fit.  Any output array may be
 * NULL (offsets included). */
int lo_iris_batch_compare_all(lo_iris_batch* ib, const int* jobs, int k, const float* const* pts_xyz, const size_t* n,
                              int on_device, size_t* offsets, float* out_dist, int32_t* out_bias, int32_t* out_diff,
                              int32_t* out_total, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* LO_IRIS_BATCH_H */
