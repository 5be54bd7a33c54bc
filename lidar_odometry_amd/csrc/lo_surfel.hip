// lo_surfel.hip — the context's device surfel table: full uploads (lo_map_set_surfels), in-place patches, the keyed
// sync, deferred surfel fits of a synced host map, and the table a device map reserves (lo_ctx_internal.h).
#include "lo_ctx_def.h"

// pack_key (lo_device.h): three 21-bit fields key + 2^20
static uint64_t pack_key_host(int32_t x, int32_t y, int32_t z) {
    return static_cast<uint64_t>(static_cast<uint32_t>(x + (1 << 20))) |
           (static_cast<uint64_t>(static_cast<uint32_t>(y + (1 << 20))) << 21) |
           (static_cast<uint64_t>(static_cast<uint32_t>(z + (1 << 20))) << 42);
}

extern "C" {

int lo_map_set_surfels(lo_ctx* c, const int32_t* keys, const float* normals, const float* centroids, size_t m) {
    if (!c) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    if (m > 0 && (!keys || !normals || !centroids)) { c->err = "null surfel arrays"; return LO_ERR_ARG; }
    size_t cap = 2;
    uint32_t l2 = 1;
    while (cap < 4 * m) { cap <<= 1; ++l2; }            // load <= 1/4: room for in-place patches up to 1/2
    std::vector<Slot> h(cap);
    for (auto& s : h) { s.key = kEmptyKey; s.n[0] = s.n[1] = s.n[2] = 0.0f; s.c[0] = s.c[1] = s.c[2] = 0.0f; }
    const uint64_t mask = cap - 1;
    std::unordered_set<uint64_t> resident;
    resident.reserve(2 * m);
    for (size_t i = 0; i < m; ++i) {
        for (int a = 0; a < 3; ++a) {
            const int32_t v = keys[3 * i + a];
            if (v < -(1 << 20) || v >= (1 << 20)) { c->err = "surfel key outside +-2^20"; return LO_ERR_ARG; }
        }
        const uint64_t key = pack_key_host(keys[3 * i], keys[3 * i + 1], keys[3 * i + 2]);
        resident.insert(key);
        uint64_t b = (key * 0x9E3779B97F4A7C15ull) >> (64 - l2);
        while (h[b].key != kEmptyKey && h[b].key != key) b = (b + 1) & mask;
        h[b].key = key;                                    // duplicate keys: last one wins (map semantics)
        for (int a = 0; a < 3; ++a) { h[b].n[a] = normals[3 * i + a]; h[b].c[a] = centroids[3 * i + a]; }
    }
    LO_HIP(c, hipSetDevice(c->device));
    LO_HIP(c, hipStreamSynchronize(c->stream));
    LO_HIP(c, c->d_tab.reserve(cap));
    LO_HIP(c, hipMemcpy(c->d_tab, h.data(), cap * sizeof(Slot), hipMemcpyHostToDevice));
    c->log2cap = l2;
    c->n_surfels = resident.size();
    c->resident.swap(resident);
    c->n_tomb = 0;
    c->map_src = 0;                                      // no longer mirrors a synced host map
    ++c->tab_gen;
    ++c->tab_edit;
    return LO_OK;
}

}  // extern "C"

namespace lo {
struct MapPatchRec {                  // one L1 voxel's change: upsert (op 1: key + payload) or erase (op 0)
    uint64_t key;
    float n[3];
    float c[3];
    uint32_t op;
    uint32_t pad;
};
void ctx_map_source(const lo_ctx* c, uint64_t* src, uint64_t* epoch, uint64_t* pos) {
    *src = c->map_src; *epoch = c->map_epoch; *pos = c->map_pos;
}
void ctx_set_map_source(lo_ctx* c, uint64_t src, uint64_t epoch, uint64_t pos) {
    c->map_src = src; c->map_epoch = epoch; c->map_pos = pos;
}

int ctx_reserve_table(lo_ctx* c, size_t min_slots, void** tab, uint32_t* log2cap, uint64_t* gen) {
    if (!c || !tab || !log2cap || !gen) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    size_t cap = 2;
    uint32_t l2 = 1;
    while (cap < min_slots) { cap <<= 1; ++l2; }
    if (c->devmap_gen != c->tab_gen || c->devmap_gen == 0 || (size_t(1) << c->log2cap) < cap) {
        LO_HIP(c, hipSetDevice(c->device));
        if (cap > c->d_tab.capacity()) {
            LO_HIP(c, hipStreamSynchronize(c->stream));
            LO_HIP(c, c->d_tab.reserve(cap));
        } else {
            cap = std::max(cap, size_t(1) << c->log2cap);   // keep the larger table
            l2 = 1;
            while ((size_t(1) << l2) < cap) ++l2;
        }
        LO_HIP(c, hipMemsetAsync(c->d_tab, 0xff, cap * sizeof(Slot), c->stream));
        c->log2cap = l2;
        c->resident.clear();
        c->n_surfels = 0;
        c->n_tomb = 0;
        c->map_src = 0;
        ++c->tab_gen;
        c->devmap_gen = c->tab_gen;
    }
    ++c->tab_edit;                                       // the device map patches the table from now on
    *tab = c->d_tab;
    *log2cap = c->log2cap;
    *gen = c->tab_gen;
    return LO_OK;
}

int ctx_filtered_device(lo_ctx* c, const float** d_pts, const int** d_n) {
    if (!c || !d_pts || !d_n) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    if (!c->last_dev_count || !c->vf.n_out) { c->err = "no device-filtered scan"; return LO_ERR_STATE; }
    *d_pts = c->d_pts;
    *d_n = c->vf.n_out;
    return LO_OK;
}

bool ctx_table_current(const lo_ctx* c, size_t min_slots) {
    return c && c->devmap_gen == c->tab_gen && c->devmap_gen != 0 && (size_t(1) << c->log2cap) >= min_slots;
}

long long ctx_filtered_count_known(const lo_ctx* c) {
    return (c && c->last_dev_count && c->nf_valid && !c->pending) ? static_cast<long long>(*c->h_nf) : -1;
}

// a pinned staging buffer and its device copy, grown together (both freed before either is allocated)
static int grow_pinned_pair(lo_ctx* c, PinnedBuf<void>& h, DevBuf<void>& d, size_t bytes) {
    if (bytes <= std::min(h.capacity(), d.capacity())) return LO_OK;
    h.reset();
    d.reset();
    const size_t b = std::max<size_t>(2 * bytes, 64 * 1024);
    LO_HIP(c, h.reserve(b));
    LO_HIP(c, d.reserve(b));
    return LO_OK;
}

// The pending fit launch's planarity failures leave the resident mirror (the kernel erased them from the table), once:
// before a count is reported, before another patch or fit reads the mirror, and when the map collects the results.
static int reconcile_fit(lo_ctx* c) {
    if (c->fit_ticket == 0 || c->fit_reconciled) return LO_OK;
    LO_HIP(c, hipSetDevice(c->device));
    LO_HIP(c, hipEventSynchronize(c->ev_fit));
    const FitResult* out = static_cast<const FitResult*>(c->h_fit_out.get());
    if (c->fit_gen == c->tab_gen)                        // the table still holds what the kernel patched
        for (size_t j = 0; j < c->fit_keys.size(); ++j)
            if (out[j].planarity > c->fit_thr) c->resident.erase(c->fit_keys[j]);
    c->n_surfels = c->resident.size();
    c->fit_reconciled = true;
    return LO_OK;
}

int ctx_fit_surfels(lo_ctx* c, const int32_t* keys, const int32_t* offs, size_t n_jobs, const float* cs, size_t n_cs,
                    float thr, uint64_t* ticket) {
    if (!c || !ticket || (n_jobs > 0 && (!keys || !offs || !cs))) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    if (!c->d_tab) { c->err = "no surfel table to patch"; return LO_ERR_STATE; }
    int rc0 = reconcile_fit(c);                          // a superseded ticket's failures must not stay resident
    if (rc0 != LO_OK) return rc0;
    if (n_jobs > static_cast<size_t>(INT32_MAX) || n_cs > static_cast<size_t>(INT32_MAX / 3)) return LO_ERR_CAPACITY;
    // worst case for the table: every job not resident inserts, every resident one leaves a tombstone
    std::vector<uint64_t> pk(n_jobs);
    size_t ins = 0, ers = 0;
    for (size_t j = 0; j < n_jobs; ++j) {
        for (int a = 0; a < 3; ++a) {
            const int32_t v = keys[3 * j + a];
            if (v < -(1 << 20) || v >= (1 << 20)) { c->err = "surfel key outside +-2^20"; return LO_ERR_ARG; }
        }
        pk[j] = pack_key_host(keys[3 * j], keys[3 * j + 1], keys[3 * j + 2]);
        if (c->resident.count(pk[j])) ++ers; else ++ins;
    }
    const size_t cap = size_t(1) << c->log2cap;
    if (c->resident.size() + ins + c->n_tomb + ers > cap / 2) { c->err = "table full"; return LO_ERR_CAPACITY; }
    LO_HIP(c, hipSetDevice(c->device));
    if (!c->ev_fit) LO_HIP(c, hipEventCreateWithFlags(&c->ev_fit, hipEventDisableTiming));
    else LO_HIP(c, hipEventSynchronize(c->ev_fit));     // the previous fit has left the staging buffers
    const size_t jb = n_jobs * sizeof(FitJob), in_bytes = jb + n_cs * 3 * sizeof(float);
    int rc = grow_pinned_pair(c, c->h_fit_in, c->d_fit_in, in_bytes);
    if (rc != LO_OK) return rc;
    rc = grow_pinned_pair(c, c->h_fit_out, c->d_fit_out, n_jobs * sizeof(FitResult));
    if (rc != LO_OK) return rc;
    FitJob* J = static_cast<FitJob*>(c->h_fit_in.get());
    for (size_t j = 0; j < n_jobs; ++j) {
        const int32_t end = j + 1 < n_jobs ? offs[j + 1] : static_cast<int32_t>(n_cs);
        J[j].key = pk[j];
        J[j].off = offs[j];
        J[j].m = end - offs[j];
    }
    std::memcpy(static_cast<char*>(c->h_fit_in.get()) + jb, cs, n_cs * 3 * sizeof(float));
    LO_HIP(c, hipMemcpyAsync(c->d_fit_in, c->h_fit_in, in_bytes, hipMemcpyHostToDevice, c->stream));
    if (n_jobs > 0)
        hipLaunchKernelGGL(k_surfel_fit, dim3(static_cast<unsigned>((n_jobs + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                           c->stream, static_cast<const FitJob*>(c->d_fit_in.get()),
                           reinterpret_cast<const float*>(static_cast<const char*>(c->d_fit_in.get()) + jb),
                           static_cast<int>(n_jobs), thr, c->d_tab, c->log2cap, static_cast<FitOut*>(c->d_fit_out.get()));
    LO_HIP(c, hipGetLastError());
    LO_HIP(c, hipMemcpyAsync(c->h_fit_out, c->d_fit_out, n_jobs * sizeof(FitResult), hipMemcpyDeviceToHost, c->stream));
    LO_HIP(c, hipEventRecord(c->ev_fit, c->stream));
    {
        std::lock_guard<std::mutex> g(g_live_mu);
        c->fit_ticket = ++g_ticket;
    }
    c->fit_gen = c->tab_gen;
    ++c->tab_edit;
    c->fit_keys.swap(pk);
    c->fit_reconciled = false;
    c->fit_thr = thr;
    // until the results are collected the mirror counts every job key as resident (erases are then always sent)
    for (uint64_t k : c->fit_keys) c->resident.insert(k);
    c->n_tomb += ers;
    c->n_surfels = c->resident.size();
    *ticket = c->fit_ticket;
    return LO_OK;
}

int ctx_fit_results(lo_ctx* c, uint64_t ticket, FitResult* out, size_t n_jobs) {
    {
        std::lock_guard<std::mutex> g(g_live_mu);
        if (!c || !g_live.count(c) || c->fit_ticket != ticket || ticket == 0) return LO_ERR_STATE;
    }
    if (c->fit_keys.size() != n_jobs) return LO_ERR_STATE;
    const int rc = reconcile_fit(c);
    if (rc != LO_OK) return rc;
    std::memcpy(out, c->h_fit_out, n_jobs * sizeof(FitResult));
    c->fit_ticket = 0;
    c->fit_keys.clear();
    return LO_OK;
}
}  // namespace lo

extern "C" {

// In-place patch of the device table (the §8b lo_map_patch_surfels): upserts claim the first empty slot of their
// probe sequence (atomic CAS) or overwrite their key's payload, erases leave a tombstone that lookups probe past.
// Asynchronous on the context stream (pinned staging, no host sync).  LO_ERR_CAPACITY when live keys + tombstones
// would exceed half the table: the caller uploads the whole map instead (lo_map_set_surfels).
int lo_map_patch_surfels(lo_ctx* c, const int32_t* keys, const float* normals, const float* centroids,
                         const uint8_t* present, size_t m) {
    if (!c) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    if (m == 0) return LO_OK;
    if (!keys || !normals || !centroids || !present) { c->err = "null patch arrays"; return LO_ERR_ARG; }
    if (!c->d_tab) { c->err = "no surfel table to patch"; return LO_ERR_STATE; }
    const int rc0 = reconcile_fit(c);
    if (rc0 != LO_OK) return rc0;
    // a key given more than once: its last record wins (as lo_map_set_surfels), the earlier ones are dropped, so the
    // device patch (one thread per record) never races two records of one key.  keep[i]: record i is its key's last
    // (a sort of (key, index) instead of a per-call hash map: the keyed sync hands over a few hundred keys per keyframe)
    std::vector<std::pair<uint64_t, uint32_t>> ord(m);
    for (size_t i = 0; i < m; ++i) {
        for (int a = 0; a < 3; ++a) {
            const int32_t v = keys[3 * i + a];
            if (v < -(1 << 20) || v >= (1 << 20)) { c->err = "surfel key outside +-2^20"; return LO_ERR_ARG; }
        }
        ord[i] = {pack_key_host(keys[3 * i], keys[3 * i + 1], keys[3 * i + 2]), static_cast<uint32_t>(i)};
    }
    std::sort(ord.begin(), ord.end());
    std::vector<uint8_t> keep(m, 0), res_of(m, 0);
    size_t ins = 0, ers = 0;
    for (size_t r = 0; r < m; ++r) {
        if (r + 1 < m && ord[r + 1].first == ord[r].first) continue;   // a later record of the key follows
        const size_t i = ord[r].second;
        keep[i] = 1;
        res_of[i] = c->resident.count(ord[r].first) != 0 ? 1 : 0;
        ins += (present[i] && !res_of[i]) ? 1 : 0;
        ers += (!present[i] && res_of[i]) ? 1 : 0;
    }
    const size_t cap = size_t(1) << c->log2cap;
    if ((c->resident.size() + ins - ers) + (c->n_tomb + ers) > cap / 2) { c->err = "table full"; return LO_ERR_CAPACITY; }
    LO_HIP(c, hipSetDevice(c->device));
    const size_t bytes = m * sizeof(MapPatchRec);
    if (!c->ev_patch) LO_HIP(c, hipEventCreateWithFlags(&c->ev_patch, hipEventDisableTiming));
    else LO_HIP(c, hipEventSynchronize(c->ev_patch));   // the previous patch's copy has left the staging buffer
    const int rc1 = grow_pinned_pair(c, c->h_patch, c->d_patch, bytes);
    if (rc1 != LO_OK) return rc1;
    MapPatchRec* r = static_cast<MapPatchRec*>(c->h_patch.get());
    int n_rec = 0;
    for (size_t i = 0; i < m; ++i) {
        if (!keep[i]) continue;                            // superseded by a later record of the key
        const uint64_t key = pack_key_host(keys[3 * i], keys[3 * i + 1], keys[3 * i + 2]);
        const bool res = res_of[i] != 0;
        if (!present[i] && !res) continue;                 // nothing on the device to remove
        MapPatchRec& q = r[n_rec++];
        q.key = key;
        q.op = present[i] ? 1u : 0u;
        q.pad = 0;
        for (int a = 0; a < 3; ++a) { q.n[a] = normals[3 * i + a]; q.c[a] = centroids[3 * i + a]; }
        if (present[i]) c->resident.insert(key); else c->resident.erase(key);
    }
    c->n_tomb += ers;
    c->n_surfels = c->resident.size();
    if (n_rec == 0) return LO_OK;
    ++c->tab_edit;
    LO_HIP(c, hipMemcpyAsync(c->d_patch, c->h_patch, n_rec * sizeof(MapPatchRec), hipMemcpyHostToDevice, c->stream));
    LO_HIP(c, hipEventRecord(c->ev_patch, c->stream));
    hipLaunchKernelGGL(k_map_patch, dim3((n_rec + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, c->d_tab,
                       c->log2cap, static_cast<const MapPatchRec*>(c->d_patch.get()), n_rec);
    LO_HIP(c, hipGetLastError());
    return LO_OK;
}

// The reference-side sync: the map's whole current surfel set, diffed on the host against the set this
// context last received through this call; only the difference goes to the device (lo_map_patch_surfels: upserts of
// new / refitted surfels, erases of the ones that left).  The first call, a table changed by anything else since, or a
// full table uploads everything (lo_map_set_surfels).  *patched = records sent, -1 after a full upload.
int lo_map_sync_surfels(lo_ctx* c, const int32_t* keys, const float* normals, const float* centroids, size_t m,
                        int* patched) {
    if (!c) return LO_ERR_ARG;
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }
    if (m > 0 && (!keys || !normals || !centroids)) { c->err = "null surfel arrays"; return LO_ERR_ARG; }
    if (c->kd) { c->err = "KDTree-mode context (lo_map_set_points)"; return LO_ERR_STATE; }
    std::unordered_map<uint64_t, size_t> in;
    in.reserve(2 * m);
    for (size_t i = 0; i < m; ++i) {
        for (int a = 0; a < 3; ++a) {
            const int32_t v = keys[3 * i + a];
            if (v < -(1 << 20) || v >= (1 << 20)) { c->err = "surfel key outside +-2^20"; return LO_ERR_ARG; }
        }
        in[pack_key_host(keys[3 * i], keys[3 * i + 1], keys[3 * i + 2])] = i;   // a repeated key: the last record
    }
    auto payload = [&](size_t i) {
        return std::array<float, 6>{normals[3 * i], normals[3 * i + 1], normals[3 * i + 2], centroids[3 * i],
                                    centroids[3 * i + 1], centroids[3 * i + 2]};
    };
    auto full = [&]() -> int {
        const int rc = lo_map_set_surfels(c, keys, normals, centroids, m);
        if (rc != LO_OK) return rc;
        c->smirror.clear();
        c->smirror.reserve(2 * in.size());
        for (const auto& kv : in) c->smirror[kv.first] = payload(kv.second);
        c->mirror_edit = c->tab_edit;
        if (patched) *patched = -1;
        return LO_OK;
    };
    if (c->mirror_edit != c->tab_edit) return full();
    std::vector<int32_t> pk;
    std::vector<float> pn, pc;
    std::vector<uint8_t> pres;
    for (const auto& kv : in) {
        const std::array<float, 6> p = payload(kv.second);
        auto it = c->smirror.find(kv.first);
        if (it != c->smirror.end() && std::memcmp(it->second.data(), p.data(), sizeof(p)) == 0) continue;   // unchanged
        const size_t i = kv.second;
        pk.insert(pk.end(), {keys[3 * i], keys[3 * i + 1], keys[3 * i + 2]});
        pn.insert(pn.end(), {p[0], p[1], p[2]});
        pc.insert(pc.end(), {p[3], p[4], p[5]});
        pres.push_back(1);
    }
    for (const auto& kv : c->smirror) {
        if (in.count(kv.first)) continue;                 // still a surfel
        const uint64_t k = kv.first;
        pk.insert(pk.end(), {static_cast<int32_t>(k & 0x1FFFFF) - (1 << 20), static_cast<int32_t>((k >> 21) & 0x1FFFFF) - (1 << 20),
                             static_cast<int32_t>((k >> 42) & 0x1FFFFF) - (1 << 20)});
        pn.insert(pn.end(), {0.0f, 0.0f, 0.0f});
        pc.insert(pc.end(), {0.0f, 0.0f, 0.0f});
        pres.push_back(0);
    }
    const size_t np = pres.size();
    if (np == 0) { if (patched) *patched = 0; return LO_OK; }
    const int rc = lo_map_patch_surfels(c, pk.data(), pn.data(), pc.data(), pres.data(), np);
    if (rc == LO_ERR_CAPACITY) return full();            // tombstones / growth: rebuild the table
    if (rc != LO_OK) return rc;
    for (size_t r = 0; r < np; ++r) {
        const uint64_t k = pack_key_host(pk[3 * r], pk[3 * r + 1], pk[3 * r + 2]);
        if (pres[r]) c->smirror[k] = {pn[3 * r], pn[3 * r + 1], pn[3 * r + 2], pc[3 * r], pc[3 * r + 1], pc[3 * r + 2]};
        else c->smirror.erase(k);
    }
    c->mirror_edit = c->tab_edit;
    if (patched) *patched = static_cast<int>(np);
    return LO_OK;
}

size_t lo_map_surfel_count(const lo_ctx* c) {
    if (!c) return 0;
    lo_ctx* w = const_cast<lo_ctx*>(c);
    if (reconcile_fit(w) != LO_OK) return 0;             // pending device fits: count their planarity failures out
    return w->n_surfels;
}

}  // extern "C"
