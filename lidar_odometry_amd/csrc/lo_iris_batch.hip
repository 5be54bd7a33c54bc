// lo_iris_batch.hip — the batched LiDAR-Iris detector (include/lo_iris_batch.h; DESIGN.md "Batched detector"): one
// descriptor database per job of an lo_batch, and every call one set of launches on the batch stream for all listed
// jobs.  The kernels are shells around the solo detector's device bodies (lo_iris_body.h):
//   k_iris_image_b      blockIdx.y = listed job; reads {points, count, image, destination slot} from a device table
//                       and also zeroes the job's destination slot, which the encode's atomic ORs need
//   k_iris_encode_b     grid (80, 4, k): image row, scale, listed job
//   k_iris_match_pairs  one workgroup per item of a host-built work list {query, entry a, entry b, out a, out b}
//   k_iris_counts_b     gathers the filtered scans' device counts of the listed jobs for one readback
// Bounded loops everywhere, no block waits on another.
//
// Stream operations per call, whatever k is (each "at most": a stage that has nothing to do is left out):
//   add      5 + 1 synchronise: staging copy of host clouds (packed in pinned memory), table upload, image memset,
//            k_iris_image_b, k_iris_encode_b
//   detect   8 + 1 synchronise: the five above for the queries, work-list upload, k_iris_match_pairs, record readback
//   the filtered scans' counts, only where the host does not know them: 3 + 1 synchronise more (pointer upload,
//   k_iris_counts_b, readback)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lo_iris_batch.h"
#include "lo_buf.h"
#include "lo_ctx_internal.h"
#include "lo_iris_body.h"

namespace lo {
namespace iris {

struct IrisJob {
    const float* pts;                // device points of the listed job's cloud
    int n;
    int pad;
    uint32_t* img;                   // its image (zero on entry)
    uint64_t* slot;                  // where its descriptor goes: a database slot, or the job's query slot
};
// entries and queries as indices into the database / query arrays; b == a and out_b < 0 for the odd last item of a query
struct IrisPair {
    uint32_t q;
    uint32_t a, b;
    int out_a, out_b;
};
struct IrisRec {
    float dist;
    int bias, diff, total;
};

__global__ void __launch_bounds__(256) k_iris_image_b(const IrisJob* __restrict__ jobs) {
    const IrisJob J = jobs[blockIdx.y];
    const int first = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    for (int i = first; i < kDescWords; i += step) J.slot[i] = 0;
    image_points(J.pts, J.n, J.img, first, step);
}

__global__ void __launch_bounds__(kThreads) k_iris_encode_b(const IrisJob* __restrict__ jobs,
                                                            const double2* __restrict__ h) {
    const IrisJob J = jobs[blockIdx.z];
    encode_row(J.img, h, reinterpret_cast<uint32_t*>(J.slot), blockIdx.x, blockIdx.y);
}

__global__ void __launch_bounds__(kThreads) k_iris_match_pairs(const IrisPair* __restrict__ list,
                                                               const uint64_t* __restrict__ db,
                                                               const uint64_t* __restrict__ queries,
                                                               IrisRec* __restrict__ out) {
    const IrisPair P = list[blockIdx.x];
    const uint64_t* ent[kEntries] = {db + static_cast<size_t>(P.a) * kDescWords,
                                     db + static_cast<size_t>(P.b) * kDescWords};
    const int dst[kEntries] = {P.out_a, P.out_b};
    match_block(queries + static_cast<size_t>(P.q) * kDescWords, ent,
                [&](int j, float dist, int bias, int diff, int total) {
                    if (dst[j] >= 0) out[dst[j]] = IrisRec{dist, bias, diff, total};
                });
}

__global__ void __launch_bounds__(256) k_iris_counts_b(const int* const* __restrict__ src, int k,
                                                       int* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < k) out[i] = *src[i];
}

}  // namespace iris
}  // namespace lo

// ================================================================================================== host side
using namespace lo;
using namespace lo::iris;

struct lo_iris_batch {
    lo_batch* batch = nullptr;
    int device = 0;
    int count = 0;                       // jobs of the batch
    size_t capacity = 0;                 // entries per job
    std::vector<std::vector<int64_t>> ids;   // per job
    std::vector<std::vector<float>> pos;
    DevBuf<uint64_t> d_db;               // count x capacity descriptors: job j's entry i is descriptor j * capacity + i
    DevBuf<uint64_t> d_q;                // count query descriptors, one per job
    DevBuf<uint32_t> d_img;              // count images, one per listed job of a call
    DevBuf<double2> d_h;
    PinnedBuf<float> h_pts;              // host clouds of one call, packed, and their device copy
    DevBuf<float> d_pts;
    PinnedBuf<IrisJob> h_tab;            // count
    DevBuf<IrisJob> d_tab;
    PinnedBuf<IrisPair> h_pairs;         // count x ceil(capacity / 2)
    DevBuf<IrisPair> d_pairs;
    PinnedBuf<IrisRec> h_rec;            // count x capacity
    DevBuf<IrisRec> d_rec;
    PinnedBuf<const int*> h_cntp;        // count: the filtered scans' device counts, gathered
    DevBuf<const int*> d_cntp;
    PinnedBuf<int> h_cnt;
    DevBuf<int> d_cnt;
    std::string err;
};

namespace {

// one listed job's cloud and where its descriptor goes
struct Cloud {
    const float* pts;
    size_t n;
    uint64_t* slot;
};

uint64_t* ib_entry(lo_iris_batch* m, int job, size_t i) {
    return m->d_db + (static_cast<size_t>(job) * m->capacity + i) * kDescWords;
}
uint64_t* ib_query(lo_iris_batch* m, int job) { return m->d_q + static_cast<size_t>(job) * kDescWords; }

// Every call starts here: the device, the batch as it is now, the job list checked.
int ib_enter(lo_iris_batch* m, const int* jobs, int k, BatchView* V) {
    LO_HIP(m, hipSetDevice(m->device));
    *V = batch_view(m->batch);
    if (V->pending) { m->err = "the batch has an optimize in flight"; return LO_ERR_STATE; }
    if (V->count != m->count) { m->err = "the batch changed size"; return LO_ERR_STATE; }
    if (k < 0 || (k > 0 && !jobs)) { m->err = "null job list"; return LO_ERR_ARG; }
    std::vector<char> seen(static_cast<size_t>(m->count), 0);
    for (int i = 0; i < k; ++i) {
        if (jobs[i] < 0 || jobs[i] >= m->count) { m->err = "job index out of range"; return LO_ERR_ARG; }
        if (seen[jobs[i]]) { m->err = "duplicate job index"; return LO_ERR_ARG; }
        seen[jobs[i]] = 1;
    }
    return LO_OK;
}

int ib_check_clouds(lo_iris_batch* m, int k, const float* const* pts, const size_t* n) {
    if (k > 0 && (!pts || !n)) { m->err = "null cloud arrays"; return LO_ERR_ARG; }
    for (int i = 0; i < k; ++i) {
        if (n[i] > 0 && !pts[i]) { m->err = "null cloud"; return LO_ERR_ARG; }
        if (n[i] > static_cast<size_t>(INT_MAX) / 3) { m->err = "too many points"; return LO_ERR_ARG; }
    }
    return LO_OK;
}

// The listed jobs' device-filtered scans: pts[i] / n[i], or a negative st[i] (and n[i] = 0) for a job that has none.
// Counts the host does not know are fetched with one gather launch, one readback and one synchronise for all of them.
int ib_scans(lo_iris_batch* m, const BatchView& V, const int* jobs, int k, std::vector<const float*>& pts,
             std::vector<size_t>& n, std::vector<int>& st) {
    hipStream_t bs = static_cast<hipStream_t>(V.stream);
    pts.assign(k, nullptr);
    n.assign(k, 0);
    st.assign(k, LO_OK);
    std::vector<int> ask;                                  // listed jobs whose count is on the device only
    for (int i = 0; i < k; ++i) {
        lo_ctx* c = V.ctx[jobs[i]];
        const int* d_n = nullptr;
        const int rc = ctx_filtered_device(c, &pts[i], &d_n);
        if (rc != LO_OK) {
            st[i] = rc;
            m->err = "job " + std::to_string(jobs[i]) + ": " + lo_last_error(c);
            continue;
        }
        const long long known = ctx_filtered_count_known(c);
        if (known >= 0) {
            n[i] = static_cast<size_t>(known);
        } else {
            m->h_cntp[ask.size()] = d_n;
            ask.push_back(i);
        }
    }
    if (!ask.empty()) {
        const int a = static_cast<int>(ask.size());
        LO_HIP(m, hipMemcpyAsync(m->d_cntp, m->h_cntp, sizeof(const int*) * a, hipMemcpyHostToDevice, bs));
        hipLaunchKernelGGL(k_iris_counts_b, dim3((a + 255) / 256), dim3(256), 0, bs, m->d_cntp.get(), a,
                           m->d_cnt.get());
        LO_HIP(m, hipGetLastError());
        LO_HIP(m, hipMemcpyAsync(m->h_cnt, m->d_cnt, sizeof(int) * a, hipMemcpyDeviceToHost, bs));
        LO_HIP(m, hipStreamSynchronize(bs));
        for (int j = 0; j < a; ++j) n[ask[j]] = static_cast<size_t>(std::max(m->h_cnt[j], 0));
    }
    for (int i = 0; i < k; ++i) {
        if (st[i] != LO_OK) continue;
        lo_config cfg;
        if (lo_get_config(V.ctx[jobs[i]], &cfg) != LO_OK || n[i] > static_cast<size_t>(std::max(cfg.max_points, 0))) {
            st[i] = LO_ERR_STATE;
            n[i] = 0;
            m->err = "job " + std::to_string(jobs[i]) + ": filtered count beyond max_points";
        }
    }
    return LO_OK;
}

// Enqueues image + encode for the clouds (all non-empty, at most one per job): host clouds are packed into pinned
// memory and copied once, the table is uploaded, the images are cleared with one memset, and the image kernel's
// blocks zero the destination slots.  No synchronise.
int ib_describe(lo_iris_batch* m, hipStream_t bs, const std::vector<Cloud>& cl, int on_device) {
    const int k = static_cast<int>(cl.size());
    if (k == 0) return LO_OK;
    std::vector<const float*> dev(k);
    if (on_device) {
        for (int a = 0; a < k; ++a) dev[a] = cl[a].pts;
    } else {
        size_t total = 0;
        for (const Cloud& c : cl) total += 3 * c.n;
        if (total > std::min(m->h_pts.capacity(), m->d_pts.capacity())) {      // nothing is in flight: calls are synchronous
            const size_t want = std::max<size_t>(2 * total, size_t(3) << 16);
            LO_HIP(m, m->h_pts.reserve(want));
            LO_HIP(m, m->d_pts.reserve(want));
        }
        size_t at = 0;
        for (int a = 0; a < k; ++a) {
            std::memcpy(m->h_pts + at, cl[a].pts, 3 * cl[a].n * sizeof(float));
            dev[a] = m->d_pts + at;
            at += 3 * cl[a].n;
        }
        LO_HIP(m, hipMemcpyAsync(m->d_pts, m->h_pts, total * sizeof(float), hipMemcpyHostToDevice, bs));
    }
    size_t max_n = 1;
    for (int a = 0; a < k; ++a) {
        m->h_tab[a] = IrisJob{dev[a], static_cast<int>(cl[a].n), 0, m->d_img + static_cast<size_t>(a) * kImgWords,
                              cl[a].slot};
        max_n = std::max(max_n, cl[a].n);
    }
    LO_HIP(m, hipMemcpyAsync(m->d_tab, m->h_tab, sizeof(IrisJob) * k, hipMemcpyHostToDevice, bs));
    LO_HIP(m, hipMemsetAsync(m->d_img, 0, static_cast<size_t>(k) * kImgWords * sizeof(uint32_t), bs));
    const unsigned blocks = static_cast<unsigned>(std::min<size_t>(1024, (max_n + 255) / 256));
    hipLaunchKernelGGL(k_iris_image_b, dim3(blocks, k), dim3(256), 0, bs, m->d_tab.get());
    hipLaunchKernelGGL(k_iris_encode_b, dim3(kRows, kScales, k), dim3(kThreads), 0, bs, m->d_tab.get(), m->d_h.get());
    LO_HIP(m, hipGetLastError());
    return LO_OK;
}

// The work list of one query: entries e[0..ne) of `job` (indices into its database), two per item, records from
// `out` on in the order of e.  Returns the number of items appended at h_pairs[at].
size_t ib_pairs(lo_iris_batch* m, size_t at, int job, const size_t* e, size_t ne, size_t out) {
    const uint32_t base = static_cast<uint32_t>(static_cast<size_t>(job) * m->capacity);
    size_t items = 0;
    for (size_t i = 0; i < ne; i += kEntries, ++items) {
        IrisPair P;
        P.q = static_cast<uint32_t>(job);
        P.a = base + static_cast<uint32_t>(e[i]);
        P.out_a = static_cast<int>(out + i);
        const bool two = i + 1 < ne;                       // an odd count: the last item repeats its entry, written once
        P.b = two ? base + static_cast<uint32_t>(e[i + 1]) : P.a;
        P.out_b = two ? static_cast<int>(out + i + 1) : -1;
        m->h_pairs[at + items] = P;
    }
    return items;
}

// Work-list upload, the match launch and the readback of n_out records.  No synchronise.
int ib_match(lo_iris_batch* m, hipStream_t bs, size_t items, size_t n_out) {
    if (items == 0) return LO_OK;
    LO_HIP(m, hipMemcpyAsync(m->d_pairs, m->h_pairs, sizeof(IrisPair) * items, hipMemcpyHostToDevice, bs));
    hipLaunchKernelGGL(k_iris_match_pairs, dim3(static_cast<unsigned>(items)), dim3(kThreads), 0, bs,
                       m->d_pairs.get(), m->d_db.get(), m->d_q.get(), m->d_rec.get());
    LO_HIP(m, hipGetLastError());
    LO_HIP(m, hipMemcpyAsync(m->h_rec, m->d_rec, sizeof(IrisRec) * n_out, hipMemcpyDeviceToHost, bs));
    return LO_OK;
}

int first_negative(const int* status, int k) {
    for (int i = 0; i < k; ++i)
        if (status[i] < 0) return status[i];
    return LO_OK;
}

// lo_iris_batch_add / _add_from_scans after their clouds are known: st holds what is already decided per job.
int ib_add(lo_iris_batch* m, const BatchView& V, const int* jobs, int k, const int64_t* ids, const float* positions,
           const float* const* pts, const size_t* n, int on_device, std::vector<int>& st) {
    std::vector<Cloud> cl;
    std::vector<int> who;
    for (int i = 0; i < k; ++i) {
        if (st[i] != LO_OK) continue;
        if (n[i] == 0) { st[i] = LO_INSUFFICIENT; continue; }
        const size_t have = m->ids[jobs[i]].size();
        if (have >= m->capacity) {
            st[i] = LO_ERR_CAPACITY;
            m->err = "job " + std::to_string(jobs[i]) + ": database full";
            continue;
        }
        cl.push_back(Cloud{pts[i], n[i], ib_entry(m, jobs[i], have)});
        who.push_back(i);
    }
    hipStream_t bs = static_cast<hipStream_t>(V.stream);
    const int rc = ib_describe(m, bs, cl, on_device);
    if (rc != LO_OK) return rc;
    if (!cl.empty()) LO_HIP(m, hipStreamSynchronize(bs));  // the callers' buffers (or the staging copy) are free again
    for (int i : who) {
        m->ids[jobs[i]].push_back(ids[i]);
        m->pos[jobs[i]].insert(m->pos[jobs[i]].end(), positions + 3 * i, positions + 3 * i + 3);
    }
    return LO_OK;
}

}  // namespace

extern "C" {

lo_iris_batch* lo_iris_batch_create(lo_batch* b, size_t capacity, int* err) {
    auto fail = [&](int rc, const char* msg, lo_iris_batch* m) -> lo_iris_batch* {
        std::fprintf(stderr, "lo_iris_batch_create: %s\n", m && !m->err.empty() ? m->err.c_str() : msg);
        delete m;
        if (err) *err = rc;
        return nullptr;
    };
    if (!b || capacity < 1) return fail(LO_ERR_ARG, "bad arguments (a batch, capacity >= 1)", nullptr);
    const BatchView V = batch_view(b);
    // entries are addressed with 32-bit indices by the work list
    if (V.count < 1 || capacity > (size_t(1) << 24) / static_cast<size_t>(V.count))
        return fail(LO_ERR_ARG, "bad arguments (jobs x capacity <= 2^24)", nullptr);
    lo_iris_batch* m = new lo_iris_batch();
    m->batch = b;
    m->device = V.device;
    m->count = V.count;
    m->capacity = capacity;
    auto init = [&]() -> int {
        LO_HIP(m, hipSetDevice(m->device));
        const size_t B = static_cast<size_t>(m->count), all = B * capacity, items = B * ((capacity + 1) / 2);
        LO_HIP(m, m->d_db.reserve(all * kDescWords));
        LO_HIP(m, m->d_q.reserve(B * kDescWords));
        LO_HIP(m, m->d_img.reserve(B * kImgWords));
        LO_HIP(m, m->d_h.reserve(static_cast<size_t>(kScales) * kCols));
        LO_HIP(m, m->h_tab.reserve(B));
        LO_HIP(m, m->d_tab.reserve(B));
        LO_HIP(m, m->h_pairs.reserve(items));
        LO_HIP(m, m->d_pairs.reserve(items));
        LO_HIP(m, m->h_rec.reserve(all));
        LO_HIP(m, m->d_rec.reserve(all));
        LO_HIP(m, m->h_cntp.reserve(B));
        LO_HIP(m, m->d_cntp.reserve(B));
        LO_HIP(m, m->h_cnt.reserve(B));
        LO_HIP(m, m->d_cnt.reserve(B));
        std::vector<double> h;
        build_kernels(h);
        LO_HIP(m, hipMemcpy(m->d_h, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
        return LO_OK;
    };
    const int rc = init();
    if (rc != LO_OK) return fail(rc, "allocation", m);
    m->ids.resize(m->count);
    m->pos.resize(m->count);
    if (err) *err = LO_OK;
    return m;
}

void lo_iris_batch_destroy(lo_iris_batch* m) {
    if (!m) return;
    (void)hipSetDevice(m->device);                         // every call was synchronous: nothing is in flight
    delete m;
}

const char* lo_iris_batch_last_error(const lo_iris_batch* m) { return m ? m->err.c_str() : "null detector"; }
size_t lo_iris_batch_size(const lo_iris_batch* m, int job) {
    return m && job >= 0 && job < m->count ? m->ids[job].size() : 0;
}
size_t lo_iris_batch_capacity(const lo_iris_batch* m) { return m ? m->capacity : 0; }

int lo_iris_batch_clear(lo_iris_batch* m, int job) {
    if (!m) return LO_ERR_ARG;
    if (job < -1 || job >= m->count) { m->err = "job index out of range"; return LO_ERR_ARG; }
    for (int j = 0; j < m->count; ++j)
        if (job < 0 || j == job) {
            m->ids[j].clear();
            m->pos[j].clear();
        }
    return LO_OK;
}

int lo_iris_batch_add(lo_iris_batch* m, const int* jobs, int k, const int64_t* ids, const float* positions,
                      const float* const* pts, const size_t* n, int on_device, int* status) {
    if (!m) return LO_ERR_ARG;
    if (k > 0 && (!ids || !positions || !status)) { m->err = "null argument"; return LO_ERR_ARG; }
    BatchView V;
    int rc = ib_enter(m, jobs, k, &V);
    if (rc == LO_OK) rc = ib_check_clouds(m, k, pts, n);
    if (rc != LO_OK) return rc;
    std::vector<int> st(k, LO_OK);
    rc = ib_add(m, V, jobs, k, ids, positions, pts, n, on_device, st);
    if (rc != LO_OK) return rc;
    std::copy(st.begin(), st.end(), status);
    return first_negative(status, k);
}

int lo_iris_batch_add_from_scans(lo_iris_batch* m, const int* jobs, int k, const int64_t* ids, const float* positions,
                                 int* status) {
    if (!m) return LO_ERR_ARG;
    if (k > 0 && (!ids || !positions || !status)) { m->err = "null argument"; return LO_ERR_ARG; }
    BatchView V;
    int rc = ib_enter(m, jobs, k, &V);
    if (rc != LO_OK) return rc;
    std::vector<const float*> pts;
    std::vector<size_t> n;
    std::vector<int> st;
    rc = ib_scans(m, V, jobs, k, pts, n, st);
    if (rc == LO_OK) rc = ib_add(m, V, jobs, k, ids, positions, pts.data(), n.data(), 1, st);
    if (rc != LO_OK) return rc;
    std::copy(st.begin(), st.end(), status);
    return first_negative(status, k);
}

int lo_iris_batch_detect(lo_iris_batch* m, const lo_iris_config* cfg, const int* jobs, int k, const int64_t* ids,
                         const float* positions, const float* const* pts, const size_t* n, int on_device,
                         lo_iris_candidate* cand, int* status) {
    if (!m) return LO_ERR_ARG;
    if (!cfg || (k > 0 && (!ids || !positions || !cand || !status))) { m->err = "null argument"; return LO_ERR_ARG; }
    BatchView V;
    int rc = ib_enter(m, jobs, k, &V);
    if (rc == LO_OK && pts) rc = ib_check_clouds(m, k, pts, n);
    if (rc != LO_OK) return rc;
    std::vector<const float*> spts;
    std::vector<size_t> sn;
    std::vector<int> st(k, LO_OK);
    if (!pts) {
        rc = ib_scans(m, V, jobs, k, spts, sn, st);
        if (rc != LO_OK) return rc;
        pts = spts.data();
        n = sn.data();
        on_device = 1;
    }
    // the gate: the entries that pass the selection rule's two distance-free tests, per listed job
    std::vector<std::vector<size_t>> elig(k);
    std::vector<Cloud> cl;
    std::vector<int> who;
    std::vector<size_t> first;                             // the job's first record
    size_t items = 0, n_out = 0;
    for (int i = 0; i < k; ++i) {
        if (st[i] != LO_OK) continue;
        st[i] = LO_INSUFFICIENT;
        const int job = jobs[i];
        const std::vector<int64_t>& jid = m->ids[job];
        if (n[i] == 0 || jid.empty()) continue;
        for (size_t e = 0; e < jid.size(); ++e)
            if (eligible(*cfg, ids[i], positions + 3 * i, jid[e], m->pos[job].data() + 3 * e)) elig[i].push_back(e);
        if (elig[i].empty()) continue;
        cl.push_back(Cloud{pts[i], n[i], ib_query(m, job)});
        who.push_back(i);
        first.push_back(n_out);
        items += ib_pairs(m, items, job, elig[i].data(), elig[i].size(), n_out);
        n_out += elig[i].size();
    }
    if (!who.empty()) {
        hipStream_t bs = static_cast<hipStream_t>(V.stream);
        rc = ib_describe(m, bs, cl, on_device);
        if (rc == LO_OK) rc = ib_match(m, bs, items, n_out);
        if (rc != LO_OK) return rc;
        LO_HIP(m, hipStreamSynchronize(bs));
    }
    // the rest of the rule on the returned distances
    for (size_t w = 0; w < who.size(); ++w) {
        const int i = who[w];
        const IrisRec* rec = m->h_rec + first[w];
        Best best;
        for (size_t x = 0; x < elig[i].size(); ++x) best.offer(static_cast<long long>(x), rec[x].dist);
        const long long x = best.pick(*cfg);
        if (x < 0) continue;
        cand[i].query_keyframe_id = ids[i];
        cand[i].match_keyframe_id = m->ids[jobs[i]][elig[i][x]];
        cand[i].distance = rec[x].dist;
        cand[i].bias = rec[x].bias;
        st[i] = LO_OK;
    }
    std::copy(st.begin(), st.end(), status);
    return first_negative(status, k);
}

int lo_iris_batch_compare_all(lo_iris_batch* m, const int* jobs, int k, const float* const* pts, const size_t* n,
                              int on_device, size_t* offsets, float* out_dist, int32_t* out_bias, int32_t* out_diff,
                              int32_t* out_total, size_t cap) {
    if (!m) return LO_ERR_ARG;
    BatchView V;
    int rc = ib_enter(m, jobs, k, &V);
    if (rc == LO_OK) rc = ib_check_clouds(m, k, pts, n);
    if (rc != LO_OK) return rc;
    std::vector<Cloud> cl;
    std::vector<size_t> all, off(static_cast<size_t>(k) + 1, 0);
    size_t items = 0;
    for (int i = 0; i < k; ++i) {
        const size_t ne = n[i] > 0 ? m->ids[jobs[i]].size() : 0;
        off[i + 1] = off[i] + ne;
        if (ne == 0) continue;
        cl.push_back(Cloud{pts[i], n[i], ib_query(m, jobs[i])});
        all.resize(std::max(all.size(), ne));
        for (size_t e = 0; e < ne; ++e) all[e] = e;
        items += ib_pairs(m, items, jobs[i], all.data(), ne, off[i]);
    }
    if (offsets) std::copy(off.begin(), off.end(), offsets);
    const size_t n_out = off[k];
    if (n_out > cap) { m->err = "the records do not fit the output arrays"; return LO_ERR_CAPACITY; }
    if (n_out == 0) return LO_OK;
    hipStream_t bs = static_cast<hipStream_t>(V.stream);
    rc = ib_describe(m, bs, cl, on_device);
    if (rc == LO_OK) rc = ib_match(m, bs, items, n_out);
    if (rc != LO_OK) return rc;
    LO_HIP(m, hipStreamSynchronize(bs));
    for (size_t x = 0; x < n_out; ++x) {
        const IrisRec& r = m->h_rec[x];
        if (out_dist) out_dist[x] = r.dist;
        if (out_bias) out_bias[x] = r.bias;
        if (out_diff) out_diff[x] = r.diff;
        if (out_total) out_total[x] = r.total;
    }
    return LO_OK;
}

}  // extern "C"
