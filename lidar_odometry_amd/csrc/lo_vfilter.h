// lo_vfilter.h — device FastVoxelFilter (lo_vfilter.hip), host-side interface for the context (lo_optimize.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "lo_buf.h"

namespace lo {

// Voxel slot of the filter's hash table: first / last sample index, member count, bucket fill cursor.
struct VfSlot {
    uint32_t first, last, cnt, fill;
};

// Device counters of one filter pass (reset by the pass itself).
struct VfCounters {
    int n_out;                   // voxels = output points (read by the ICP kernels as KParams::n_dev)
    unsigned arrive;             // (unused since r06: no last-block hand-off)
    int n_mid, n_big;            // voxels with 17..64 / more than 64 samples (k_vf_wide)
};

struct VfBuffers {
    size_t cap = 0;              // samples
    size_t tcap = 0;             // table slots (power of two >= 2 * cap)
    DevBuf<uint64_t> tkey;       // table keys (kVfEmpty = free)
    DevBuf<VfSlot> tslot;
    DevBuf<int32_t> sslot;       // per sample: table slot, -1 = non-finite point
    DevBuf<float> samp;          // per sample: its point (compact AoS float3; the raw scan is read once)
    DevBuf<int2> loc;            // per head sample: (output slot, bucket start) inside its k_vf_heads block
    DevBuf<int2> blk;            // per k_vf_heads block: (heads, members)
    DevBuf<int2> blk_pre;        // their exclusive prefix (+ the total), published by k_vf_place's block 0
    DevBuf<int32_t> bucket;      // members of each voxel (bucket order = arrival order; sorted when summed)
    DevBuf<int32_t> mid;         // head samples of voxels with 17..64 members
    DevBuf<int32_t> big;         // head samples of voxels with more than 64 members
    DevBuf<VfCounters> ctr;
    int* n_out = nullptr;        // &ctr->n_out
};

// One job of the batched filter (k_vf_*_b): what the single-scan launches take as arguments, in device memory.
struct VfJob {
    const float* raw;            // device memory or the device alias of pinned host memory (null when m = 0)
    int m;                       // samples = ceil(n_raw / stride)
    int l2;                      // log2 of the table size
    uint64_t mask;               // table size - 1
    uint64_t* tkey;
    VfSlot* tslot;
    int32_t* sslot;
    float* samp;
    int2* loc;
    int2* blk;
    int2* blk_pre;
    int32_t* bucket;
    int32_t* mid;
    int32_t* big;
    VfCounters* ctr;
    float* out;                  // the job's filtered cloud (its context's d_pts)
};

hipError_t vf_reserve(VfBuffers& b, size_t m, hipStream_t s);
// Filter d_raw (n_raw AoS float3) into d_out on stream s; the output count lands in b.n_out (device).
// m_out = ceil(n_raw / stride), an upper bound of the output count.
hipError_t vf_enqueue(VfBuffers& b, const float* d_raw, size_t n_raw, int stride, float voxel_size, float* d_out,
                      hipStream_t s, int& m_out);

// The descriptor of a job of m samples on buffers b (reserved for at least m samples), output into d_out.
VfJob vf_job(const VfBuffers& b, const float* d_raw, size_t m, float* d_out);
// Enqueue the filter of B jobs (d_jobs: their descriptors in device memory; max_m: the largest job's samples) on
// stream s: five batched launches.  Job j's count lands in its counters' n_out and in d_counts[j].
hipError_t vf_enqueue_batch(const VfJob* d_jobs, int B, size_t max_m, int stride, float voxel_size, int* d_counts,
                            hipStream_t s);

}  // namespace lo
