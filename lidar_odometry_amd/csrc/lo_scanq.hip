// lo_scanq.hip — the scan queue (ScanQueue, lo_scanq.h): the lanes' buffers, the pending holds, recovery after a
// timed-out wait, the snapshot / apply / emit steps around plan_scan (lo_scan_plan.h), and the queue's entry points.
#include <atomic>

#include "lo_ctx_def.h"
#include "lo_lockstep.h"

namespace lo {
// ---------------------------------------------------------------- lanes
int lane_alloc_base(lo_ctx* c, ScanLane& L) {
    const size_t NB = (static_cast<size_t>(c->cfg.max_points) + kBlock - 1) / kBlock;
    LO_HIP(c, L.d_slot.reserve(NB * kBlock));
    LO_HIP(c, L.d_res_pko.reserve(NB * kBlock));
    LO_HIP(c, L.d_wmask.reserve(NB * kWavesPerBlock));
    LO_HIP(c, L.d_blk_cnt.reserve(NB));
    LO_HIP(c, L.d_blk_sum.reserve(NB));
    LO_HIP(c, L.d_blk_m2.reserve(NB));
    LO_HIP(c, L.d_blk_part.reserve(NB * kNE));
    LO_HIP(c, L.d_js.reserve(kMaxAlpha + 1));
    LO_HIP(c, L.d_st.reserve(1));
    return LO_OK;
}
int lane_alloc_cand(lo_ctx* c, ScanLane& L) {
    const size_t cand = static_cast<size_t>(c->cfg.num_alpha_segments) + 1;
    LO_HIP(c, L.d_cand_rec.reserve(cand * kCandWords));
    LO_HIP(c, L.d_cand_cnt.reserve(cand));
    LO_HIP(c, L.d_acc_part.reserve(cand * kFuseMaxBlocks * kNE));   // last: ensure_acc_part reads it as "all three"
    return LO_OK;
}

// Lane `to` becomes the current one, with a full set of the per-scan state from its first use on.
// Depth 1: nothing of that lane is in flight, its last scan's hold was enqueued before the scan now pending started.
// Depth >= 2: that hold may still be pending, and apply_plan enqueues it before anything touches the lane.
static int lane_switch(lo_ctx* c, int to) {
    ScanQueue& q = c->q;
    ScanLane& A = q.lanes[to];
    if (!q.lane_ready[to]) {
        int rc = lane_alloc_base(c, A);
        if (rc != LO_OK) return rc;
        LO_HIP(c, hipMemsetAsync(A.d_st, 0, sizeof(DevState), c->stream));
        if ((rc = lane_alloc_cand(c, A)) != LO_OK) return rc;
        // zeroed on the context stream: this scan's head follows there, and its tail starts only behind its main part
        LO_HIP(c, hipMemsetAsync(A.d_cand_cnt, 0, A.d_cand_cnt.capacity() * sizeof(unsigned), c->stream));
        q.lane_ready[to] = true;
    }
    q.lane = to;
    ++c->cfg_gen;                                       // a batch's cached device KParams name the other lane's buffers
    return LO_OK;
}

// ---------------------------------------------------------------- pipeline state, recovery
// First pipelined scan: the first lane's tail stream, the fence words, the record ring, the host flag.
static int pipe_alloc(lo_ctx* c) {
    ScanQueue& q = c->q;
    if (q.d_hbroken) return LO_OK;                  // set last
    // (another lane's tail stream is made when a scan first runs there with two or more in flight)
    if (!q.s_tail[0]) LO_HIP(c, hipStreamCreateWithFlags(&q.s_tail[0], hipStreamNonBlocking));
    // (pipe_fail finds every group from any one: kMaxLanes x 16 bytes, aligned to that -- hipMalloc aligns to 256)
    LO_HIP(c, q.d_fin.reserve(kMaxLanes * kFinWords));
    LO_HIP(c, hipMemset(q.d_fin, 0, kMaxLanes * kFinWords * sizeof(uint32_t)));
    LO_HIP(c, q.d_ring.reserve(static_cast<size_t>(kRingRecords) * kRecWords));
    LO_HIP(c, hipMemset(q.d_ring, 0, static_cast<size_t>(kRingRecords) * kRecWords * sizeof(float)));
    LO_HIP(c, q.h_broken.reserve(1));
    *q.h_broken = 0;
    LO_HIP(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&q.d_hbroken), q.h_broken, 0));
    LO_HIP(c, hipDeviceSynchronize());              // zeroed before either stream's first poll
    return LO_OK;
}

// A pipeline wait timed out (the dispatcher ran the streams out of submission order): drain the context stream and every
// lane stream, switch the pipeline off for this context, clear the flag words.  Scans enqueued before this point report
// LO_ERR_PIPELINE (their tails left without touching anything); a synchronous call re-runs its scan on one stream
// (lo_icp_result).
int pipe_recover(lo_ctx* c) {
    ScanQueue& q = c->q;
    LO_HIP(c, sync_all(c));                         // (enqueues the pending holds of every lane first: they give up at once)
    q.pipe = false;
    ++q.pipe_timeouts;
    q.ring_n = 0;                                   // (the records of the scans that gave up were never written)
    c->err = "scan pipeline: a device-side wait timed out (the streams were not run concurrently, e.g. rocprofv3 "
             "counter collection); pipeline switched off for this context";
    LO_HIP(c, hipMemset(q.d_fin, 0, kMaxLanes * kFinWords * sizeof(uint32_t)));
    for (uint32_t& s : q.lane_seq) s = 0;           // (with the words they count in)
    LO_HIP(c, hipStreamSynchronize(nullptr));
    __atomic_store_n(q.h_broken.get(), 0u, __ATOMIC_RELEASE);
    return LO_OK;
}

// ---------------------------------------------------------------- holds
// Contexts of this process with a hold pending, i.e. with queued scans in flight right now.
static std::atomic<int> g_holding{0};
static bool group_active(const ScanGroups& g) { return g.open_n > 0 || g.slot[0].unjoined || g.slot[1].unjoined; }
// (called wherever the pending holds or the groups' state change)
static void holding_sync(lo_ctx* c) {
    ScanQueue& q = c->q;
    const bool now = q.n_hold > 0 || group_active(q.grp);
    if (now == q.grp.active) return;
    q.grp.active = now;
    g_holding.fetch_add(now ? 1 : -1, std::memory_order_relaxed);
}
// The one place a pending hold leaves the host -- the oldest one, on the context stream.  The wait is bounded by
// pipe_bound, it gives up at once when the pipeline is broken, and a timeout marks the held scan's own DevState (its
// lane's) LO_ERR_PIPELINE.
static int pop_hold(lo_ctx* c) {
    ScanQueue& q = c->q;
    const ScanQueue::Hold h = q.holds[0];
    for (int i = 1; i < q.n_hold; ++i) q.holds[i - 1] = q.holds[i];
    --q.n_hold;
    holding_sync(c);
    LO_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_wait_final, dim3(1), dim3(kWave), 0, c->stream, q.d_fin + kFinWords * h.lane, h.seq, h.st,
                       q.d_hbroken, q.pipe_bound);
    LO_HIP(c, hipGetLastError());
    return LO_OK;
}
// All pending holds, oldest first.  Called at the top of every entry point that enqueues on the context stream, reads
// from it, or changes what a queued scan reads (and by sync_all); a queue of scans places its holds by plan (apply_plan).
int flush_hold(lo_ctx* c) {
    if (group_active(c->q.grp)) {                       // the open group leaves, and the context stream waits for the slots
        const int rc = group_flush(c);
        if (rc != LO_OK) return rc;
    }
    while (c->q.n_hold > 0) {
        const int rc = pop_hold(c);
        if (rc != LO_OK) return rc;
    }
    return LO_OK;
}

// ---------------------------------------------------------------- scan groups (lo_scan_group_plan.h)
// First grouped scan of the context: the slots' streams, events and staging, the completion words, the record ring.
static int group_alloc(lo_ctx* c) {
    ScanGroups& g = c->q.grp;
    if (g.ready) return LO_OK;
    const int rc = pipe_alloc(c);                       // (the record ring)
    if (rc != LO_OK) return rc;
    for (GroupSlot& S : g.slot) {
        if (!S.s) LO_HIP(c, hipStreamCreateWithFlags(&S.s, hipStreamNonBlocking));
        LO_HIP(c, S.h_Ps.reserve(kMaxGroup));
        LO_HIP(c, S.d_P.reserve(kMaxGroup));
        LO_HIP(c, S.h_T0.reserve(12 * kMaxGroup));
        LO_HIP(c, S.d_T0.reserve(12 * kMaxGroup));
        if (!S.ev_up) LO_HIP(c, hipEventCreateWithFlags(&S.ev_up, hipEventDisableTiming));
        if (!S.ev_done) LO_HIP(c, hipEventCreateWithFlags(&S.ev_done, hipEventDisableTiming));
    }
    if (!g.ev_ring) LO_HIP(c, hipEventCreateWithFlags(&g.ev_ring, hipEventDisableTiming));
    LO_HIP(c, g.h_done.reserve(kGroupSlots));
    for (int i = 0; i < kGroupSlots; ++i) g.h_done[i] = 0;
    LO_HIP(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&g.d_hdone), g.h_done, 0));
    LO_HIP(c, lockstep_prepare());
    g.ready = true;
    return LO_OK;
}

void group_release(lo_ctx* c) {
    ScanGroups& g = c->q.grp;
    for (GroupSlot& S : g.slot) {
        if (S.s) { (void)hipStreamSynchronize(S.s); (void)hipStreamDestroy(S.s); S.s = nullptr; }
        if (S.ev_up) (void)hipEventDestroy(S.ev_up);
        if (S.ev_done) (void)hipEventDestroy(S.ev_done);
        S.ev_up = S.ev_done = nullptr;
    }
    if (g.ev_ring) (void)hipEventDestroy(g.ev_ring);
    g.ev_ring = nullptr;
    if (g.active) { g.active = false; g_holding.fetch_sub(1, std::memory_order_relaxed); }
}

hipError_t group_sync(lo_ctx* c) {
    for (GroupSlot& S : c->q.grp.slot)
        if (S.s) { const hipError_t e = hipStreamSynchronize(S.s); if (e != hipSuccess) return e; }
    return hipSuccess;
}

GroupPlanIn group_snapshot(const lo_ctx* c, size_t n, bool cand, bool timed, bool dev_count) {
    const ScanQueue& q = c->q;
    GroupPlanIn in{};
    in.scan = scan_snapshot(c, cand, timed, dev_count);
    in.group = q.grp.setting;
    in.fail_hook = q.pipe_fail_at != 0;
    in.exact = c->exact;
    in.n = static_cast<int>(std::min<size_t>(n, 0x7fffffff));
    in.merge_max = kExactMergeMax;
    in.open_n = q.grp.open_n;
    in.open_slot = q.grp.open_slot;
    in.in_flight = q.n_hold > 0 || q.grp.in_flight();
    for (int i = 0; i < kGroupSlots; ++i) in.staging_busy[i] = q.grp.slot[i].up_pending;
    return in;
}

// The scan joins the open group: the slot's next set of per-scan state becomes the current one (cur(c): lo_icp_result
// and lo_icp_export_pose read the last enqueued scan's), its KParams are made as a single scan's are.  No launch.
int group_append(lo_ctx* c, const GroupPlan& plan, const float* d_pts, size_t n, const float T_init[12]) {
    ScanGroups& g = c->q.grp;
    int rc = group_alloc(c);
    if (rc != LO_OK) return rc;
    GroupSlot& S = g.slot[g.open_slot];
    if (plan.wait_staging) {
        LO_HIP(c, hipEventSynchronize(S.ev_up));
        S.up_pending = false;
    }
    const int a = g.open_n;
    if (a >= S.n_sets) {
        if ((rc = lane_alloc_base(c, S.sets[a])) != LO_OK) return rc;
        LO_HIP(c, hipMemsetAsync(S.sets[a].d_st, 0, sizeof(DevState), S.s));
        S.n_sets = a + 1;
    }
    g.prev = g.cur;
    g.cur = &S.sets[a];
    ++c->cfg_gen;                                       // a batch's cached device KParams name another set's buffers
    GroupJob& J = g.jobs[a];
    J.pts = d_pts;
    J.n = static_cast<int>(n);
    J.exact = c->exact;
    std::memcpy(J.T0, T_init, sizeof(J.T0));
    J.P = make_params(c, d_pts, static_cast<int>(n));
    if (J.exact) J.P.scale_given = 1;                   // the scale comes from k_exact_scale_cb (iteration 0)
    g.open_n = a + 1;
    holding_sync(c);
    return LO_OK;
}

// The open group leaves: two uploads, the lockstep launch list, one export kernel -- all on the slot's stream, behind
// the slot's previous group.  A partial group below kGroupLockstepMin scans goes down the ring scan by scan instead.
int group_emit(lo_ctx* c) {
    ScanQueue& q = c->q;
    ScanGroups& g = q.grp;
    const int n = g.open_n;
    if (n == 0) return LO_OK;
    g.open_n = 0;                                       // (first: a flush_hold below finds no open group)
    if (!group_lockstep(n, group_size(g.setting))) {
        // (each replayed scan first puts the context stream behind the groups still running: enqueue_ring, group_join;
        // never timed, whatever call sends the group out)
        const bool sync_call = c->sync_call;
        c->sync_call = false;
        int rc = LO_OK;
        for (int j = 0; rc == LO_OK && j < n; ++j) {
            rc = enqueue_ring(c, g.jobs[j].pts, static_cast<size_t>(g.jobs[j].n), g.jobs[j].T0, nullptr);
            if (rc != LO_OK)
                c->err = "scan group: queued scan " + std::to_string(j + 1) + " of " + std::to_string(n) +
                         " failed on its way down the ring (it and the scans queued behind it were dropped): " + c->err;
        }
        c->sync_call = sync_call;
        holding_sync(c);
        return rc;
    }
    const int slot = g.open_slot;
    GroupSlot& S = g.slot[slot];
    LO_HIP(c, hipSetDevice(c->device));
    // The ring's pending holds first, then this group behind everything on the context stream, by one event: a queued
    // scan runs behind what the caller or the library enqueued there before it (an asynchronous table patch, a device
    // map update, the kernel that produced its points), and a ring scan 64 records back has written its record before
    // this group writes that slot of the record ring.
    while (q.n_hold > 0) {
        const int rc = pop_hold(c);
        if (rc != LO_OK) return rc;
    }
    LO_HIP(c, hipEventRecord(g.ev_ring, c->stream));
    LO_HIP(c, hipStreamWaitEvent(S.s, g.ev_ring, 0));
    // lockstep order: the fast-mode jobs, then the reference-exact ones (lo_set_exact is a flush point, so a group has
    // one mode in practice; the layout is the batch's anyway).  Records go to the ring in enqueue order.
    LockstepShape sh;
    int k = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int j = 0; j < n; ++j) {
            const GroupJob& J = g.jobs[j];
            if (J.exact != (pass == 1)) continue;
            KParams P = J.P;
            P.T0p = S.d_T0 + 12 * k;
            P.rec = q.d_ring + static_cast<size_t>((q.ring_pos + static_cast<unsigned long long>(j)) % kRingRecords) * kRecWords;
            if (pass) { ++sh.nexl; sh.n_max_ex = std::max(sh.n_max_ex, P.n); }
            else { ++sh.nfast; sh.max_acc = std::max(sh.max_acc, P.nb_acc); }
            sh.max_nb = std::max(sh.max_nb, P.nb);
            S.h_Ps[k] = P;
            std::memcpy(S.h_T0 + 12 * k, J.T0, sizeof(float) * 12);
            ++k;
        }
    }
    q.ring_pos += static_cast<unsigned long long>(n);
    q.ring_n = std::min<unsigned>(q.ring_n + static_cast<unsigned>(n), kRingRecords);
    sh.pko_wgs = std::max(1, std::min(pko_grid(c->cfg), g.pko_budget / n));
    LO_HIP(c, hipMemcpyAsync(S.d_T0, S.h_T0, sizeof(float) * 12 * n, hipMemcpyHostToDevice, S.s));
    LO_HIP(c, hipMemcpyAsync(S.d_P, S.h_Ps, sizeof(KParams) * n, hipMemcpyHostToDevice, S.s));
    LO_HIP(c, hipEventRecord(S.ev_up, S.s));
    S.up_pending = true;
    LO_HIP(c, launch_lockstep(S.s, S.d_P, sh, c->cfg.max_iterations));
    if (++S.seq == 0) S.seq = 1;                        // (0: no group yet)
    hipLaunchKernelGGL(k_export_group, dim3(1), dim3(kBlock), 0, S.s, S.d_P.get(), n, g.d_hdone + slot, S.seq);
    LO_HIP(c, hipGetLastError());
    S.unjoined = true;
    ++g.n_groups;
    g.n_scans += static_cast<unsigned long long>(n);
    q.overlapped += static_cast<unsigned long long>(n);  // none of them waits for the scan queued before it
    g.open_slot = (slot + 1) % kGroupSlots;
    holding_sync(c);
    return LO_OK;
}

// A flush point: the open group out, then the context stream behind every slot's last group -- whatever follows on it
// (a result copy, a map change, another scan) finds the grouped scans done.
int group_flush(lo_ctx* c) {
    const int rc = group_emit(c);
    return rc != LO_OK ? rc : group_join(c);
}

// The context stream behind every slot's last group (one event each; nothing to do when no group has been launched
// since the last join).  flush_hold ends with it, and every ring-path scan starts with it (enqueue_ring): the ring and
// the groups share the record ring, whose slots are written in enqueue order, so a ring scan may not finish before a
// group 64 records back has exported.
int group_join(lo_ctx* c) {
    for (GroupSlot& S : c->q.grp.slot) {
        if (!S.unjoined) continue;
        LO_HIP(c, hipEventRecord(S.ev_done, S.s));
        LO_HIP(c, hipStreamWaitEvent(c->stream, S.ev_done, 0));
        S.unjoined = false;
    }
    holding_sync(c);
    return LO_OK;
}

// ---------------------------------------------------------------- snapshot, apply, emit
ScanPlanIn scan_snapshot(const lo_ctx* c, bool cand, bool timed, bool dev_count) {
    const ScanQueue& q = c->q;
    ScanPlanIn in{};
    in.depth = q.depth;
    in.depth_used = q.depth_used;
    in.depth_auto = q.depth_auto;
    in.others_holding = g_holding.load(std::memory_order_relaxed) - (q.grp.active ? 1 : 0);
    in.pipe = q.pipe;
    in.overlap = q.overlap;
    in.pipe_main = q.pipe_main;
    in.pipe_main_auto = q.pipe_main_auto;
    in.lane = q.lane;
    in.n_hold = q.n_hold;
    for (int i = 0; i < q.n_hold; ++i) in.hold_lane[i] = q.holds[i].lane;
    in.cand = cand;
    in.kd = c->kd;
    in.timed = timed;
    in.stage_timing = c->stage_timing;
    in.dev_count = dev_count;
    in.flagged = q.flagged();
    in.max_iterations = c->cfg.max_iterations;
    return in;
}

// What the plan asks for in front of the scan's head: the flush, the lane switch, the holds that go first.
int apply_plan(lo_ctx* c, const ScanPlan& plan) {
    ScanQueue& q = c->q;
    if (plan.flush_before) {
        const int rc = flush_hold(c);
        if (rc != LO_OK) return rc;
    }
    q.depth_used = plan.depth;
    if (plan.lane == q.lane) return LO_OK;
    const int from = q.lane;
    int rc = lane_switch(c, plan.lane);
    for (int i = 0; rc == LO_OK && i < plan.pops_before_head; ++i) rc = pop_hold(c);
    if (rc == LO_OK) q.prev_lane = from;
    return rc;
}

// The launches of a pipelined scan, in the order lo_scan_plan.h argues: iterations < plan.split on the context stream,
// the rest on the tail stream behind a device-side wait for the main part; k_wait_final then holds the context stream
// until the scan's result is final -- now, or as a hold left pending.  ring_run: the pipelined scans queued back to back
// before this one.
int emit_pipelined(lo_ctx* c, const ScanPlan& plan, KParams& P, KParams& P0, int n2, unsigned ring_run) {
    ScanQueue& q = c->q;
    const int iters = c->cfg.max_iterations;
    const int rc2 = pipe_alloc(c);
    if (rc2 != LO_OK) return rc2;
    if (++q.pipe_seq == 0) q.pipe_seq = 1;                // (the test hook's count: LO_PIPE_FAIL_AT is never 0)
    const bool fail = q.pipe_fail_at != 0 && q.pipe_seq == q.pipe_fail_at;
    const int lane = q.lane;
    if (++q.lane_seq[lane] == 0) q.lane_seq[lane] = 1;    // 0 is the fence word's reset value, never a scan's number
    const uint32_t seq = q.lane_seq[lane];
    uint32_t* const fin = q.d_fin + kFinWords * lane;
    DevState* const st = cur(c).d_st;
    const int tl = plan.tail_stream;
    if (!q.s_tail[tl]) LO_HIP(c, hipStreamCreateWithFlags(&q.s_tail[tl], hipStreamNonBlocking));
    const hipStream_t s_tail = q.s_tail[tl];
    P.fin = P0.fin = fin;
    P.seq = P0.seq = seq;
    P.rec = P0.rec = q.d_ring + static_cast<size_t>(q.ring_pos % kRingRecords) * kRecWords;
    ++q.ring_pos;
    q.ring_n = std::min<unsigned>(ring_run + 1, kRingRecords);
    KParams Pt = P;                                       // tail launches: leave once scan seq is final (the
    Pt.tail = 1;                                          // DevState may already be the next scan's)
    KParams Ph = P;                                       // the main part's last pick signals the tail (signal_main)
    Ph.hold = 1;
    launch_correspond_first(c, P0, false);
    if (c->exact) launch_exact_scale_any(c, P, n2, c->stream);
    // split 0: no pick of a main part to say so -- "head done" is one more launch behind the head (the head's stores are
    // out when it starts; it releases and sets the lane's word).  The context stream is not the bound once the
    // iterations have left it.
    if (plan.signal_main) hipLaunchKernelGGL(k_signal_main, dim3(1), dim3(kWave), 0, c->stream, fin, seq);
    if (plan.overlaps) ++q.overlapped;                    // its head went in front of the previous scan's hold
    if (plan.flush_after_head) {                          // one scan in flight: that hold now, behind this scan's head
        const int rcf = flush_hold(c);
        if (rcf != LO_OK) return rcf;
    }
    for (int it = 0; it < iters; ++it) {
        const bool tail = it >= plan.split;
        if (it == plan.split)                             // bound 0: the test hook's forced timeout
            hipLaunchKernelGGL(k_wait_seq, dim3(1), dim3(kWave), 0, s_tail, fin, seq, st, q.d_hbroken,
                               fail ? 0ull : q.pipe_bound);
        const hipStream_t s = tail ? s_tail : c->stream;
        const KParams& Pi = tail ? Pt : (it + 1 == plan.split ? Ph : P);
        launch_pko_spec(c, Pi, it, s);
        if (it + 1 < iters) hipLaunchKernelGGL(k_pick_correspond, dim3(P.nb), dim3(kBlock), 0, s, Pi, it);
        else hipLaunchKernelGGL(k_pick, dim3(1), dim3(kBlock), 0, s, Pi, it);
    }
    if (plan.push_hold) {                                 // enqueued by a later pipelined scan, or by flush_hold
        q.holds[q.n_hold++] = ScanQueue::Hold{seq, lane, st};
        holding_sync(c);
    } else {
        const int rcf = flush_hold(c);                    // (none pending: a scan that does not defer flushed them above)
        if (rcf != LO_OK) return rcf;
        hipLaunchKernelGGL(k_wait_final, dim3(1), dim3(kWave), 0, c->stream, fin, seq, st, q.d_hbroken, q.pipe_bound);
    }
    LO_HIP(c, hipGetLastError());
    if (c->last_timed) LO_HIP(c, hipEventRecord(c->ev1, c->stream));
    c->pending = true;
    return LO_OK;
}

void ScanQueue::from_env() {
    // rocprofv3 counter collection serialises dispatches across queues, which the pipeline's device-side waits cannot
    // survive (k_wait_final): the pipeline starts off under it unless LO_PIPE says otherwise
    if (const char* cc = std::getenv("ROCPROF_COUNTER_COLLECTION")) {
        if (*cc && std::strcmp(cc, "0") != 0 && std::strcmp(cc, "False") != 0 && std::strcmp(cc, "false") != 0) pipe = false;
    }
    if (const char* pp = std::getenv("LO_PIPE")) pipe = std::atoi(pp) != 0;
    // (0: split 0, every GN iteration of a scan on its lane's stream)
    if (const char* pm = std::getenv("LO_PIPE_MAIN")) { pipe_main = std::max(0, std::atoi(pm)); pipe_main_auto = false; }
    if (const char* po = std::getenv("LO_OVERLAP")) overlap = std::atoi(po) != 0;
    if (const char* pd = std::getenv("LO_OVERLAP_DEPTH")) {
        depth = std::min(std::max(std::atoi(pd), 1), kMaxLanes);
        depth_auto = false;
    }
    depth_used = depth;
    if (const char* pw = std::getenv("LO_PIPE_WAIT_MS")) pipe_bound = 100000ull * std::max(1, std::atoi(pw));
    if (const char* pf = std::getenv("LO_PIPE_FAIL_AT")) pipe_fail_at = static_cast<uint32_t>(std::max(0, std::atoi(pf)));
    if (const char* pg = std::getenv("LO_SCAN_GROUP")) grp.setting = std::min(std::max(std::atoi(pg), 0), kMaxGroup);
    if (const char* pw = std::getenv("LO_SCAN_GROUP_PKO_WGS")) grp.pko_budget = std::max(1, std::atoi(pw));
}
}  // namespace lo

// lo_set_scan_depth (1..2) and lo_set_scan_lanes (1..kMaxLanes): scans in flight, scan k of a queue on lane k % depth.
// From 3 on a queue's scans take split 0 unless a split was chosen (plan_scan).
static int set_depth(lo_ctx* c, int depth, int most) {
    if (!c || depth < 1 || depth > most) return LO_ERR_ARG;
    const int rc = flush_hold(c);
    if (rc != LO_OK) return rc;
    c->q.depth = depth;
    c->q.depth_auto = false;
    return LO_OK;
}

extern "C" {

int lo_icp_flush(lo_ctx* c) {
    if (!c) return LO_ERR_ARG;
    return flush_hold(c);
}

int lo_icp_queue_records(lo_ctx* c, int n_last, float* out16xN) {
    if (!c || n_last < 0 || (n_last > 0 && !out16xN)) return LO_ERR_ARG;
    ScanQueue& q = c->q;
    LO_HIP(c, hipSetDevice(c->device));
    { const int rcf = flush_hold(c); if (rcf != LO_OK) return rcf; }   // (the open group's scans get their slots here)
    if (n_last > kRingRecords || static_cast<unsigned>(n_last) > q.ring_n) {
        c->err = "lo_icp_queue_records: n_last exceeds the ring, or the pipelined scans queued since the last other call";
        return LO_ERR_ARG;
    }
    LO_HIP(c, hipSetDevice(c->device));
    LO_HIP(c, sync_all(c));                              // the holds, then every stream of the context
    if (q.flagged()) {                                   // a wait timed out: those scans' records were never written
        const int rc = pipe_recover(c);
        return rc != LO_OK ? rc : LO_ERR_PIPELINE;
    }
    const unsigned long long first = q.ring_pos - static_cast<unsigned long long>(n_last);
    // oldest first: the run up to the ring's end, then the wrapped rest
    const size_t slot = static_cast<size_t>(first % kRingRecords);
    const size_t run = std::min<size_t>(static_cast<size_t>(n_last), kRingRecords - slot);
    if (run > 0)
        LO_HIP(c, hipMemcpy(out16xN, q.d_ring + slot * kRecWords, run * kRecWords * sizeof(float), hipMemcpyDeviceToHost));
    if (run < static_cast<size_t>(n_last))
        LO_HIP(c, hipMemcpy(out16xN + run * kRecWords, q.d_ring.get(), (n_last - run) * kRecWords * sizeof(float),
                            hipMemcpyDeviceToHost));
    return LO_OK;
}

int lo_pipeline_status(lo_ctx* c, int out[4]) {
    if (!c || !out) return LO_ERR_ARG;
    out[0] = c->q.pipe ? 1 : 0;
    out[1] = c->q.pipe_main;
    out[2] = static_cast<int>(c->q.pipe_timeouts);
    out[3] = static_cast<int>(c->q.pipe_reruns);
    return LO_OK;
}

int lo_set_pipeline(lo_ctx* c, int enable, int main_iterations) {
    if (!c || main_iterations < 0) return LO_ERR_ARG;
    const int rc = flush_hold(c);
    if (rc != LO_OK) return rc;
    c->q.pipe = enable != 0;
    if (main_iterations > 0) { c->q.pipe_main = main_iterations; c->q.pipe_main_auto = false; }
    return LO_OK;
}

int lo_set_scan_overlap(lo_ctx* c, int enable) {
    if (!c) return LO_ERR_ARG;
    const int rc = flush_hold(c);
    if (rc != LO_OK) return rc;
    c->q.overlap = enable != 0;
    return LO_OK;
}

int lo_set_scan_depth(lo_ctx* c, int depth) { return set_depth(c, depth, 2); }
int lo_set_scan_lanes(lo_ctx* c, int lanes) { return set_depth(c, lanes, kMaxLanes); }

// Scans per lockstep group of a queue (lo_scan_group_plan.h): 0 the default, 1 off (every queued scan down the ring).
int lo_set_scan_group(lo_ctx* c, int group) {
    if (!c || group < 0 || group > kMaxGroup) return LO_ERR_ARG;
    const int rc = flush_hold(c);
    if (rc != LO_OK) return rc;
    c->q.grp.setting = group;
    return LO_OK;
}

int lo_scan_group_status(lo_ctx* c, long long out[4]) {
    if (!c || !out) return LO_ERR_ARG;
    out[0] = group_size(c->q.grp.setting);
    out[1] = static_cast<long long>(c->q.grp.n_groups);
    out[2] = static_cast<long long>(c->q.grp.n_scans);
    out[3] = c->q.grp.open_n;
    return LO_OK;
}

int lo_scan_overlap_status(lo_ctx* c, long long out[2]) {
    if (!c || !out) return LO_ERR_ARG;
    out[0] = c->q.overlap ? 1 : 0;
    out[1] = static_cast<long long>(c->q.overlapped);
    return LO_OK;
}

}  // extern "C"
