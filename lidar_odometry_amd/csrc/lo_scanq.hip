// lo_scanq.hip — the scan queue (ScanQueue, lo_scanq.h): the lanes' buffers, the pending holds, recovery after a
// timed-out wait, the snapshot / apply / emit steps around plan_scan (lo_scan_plan.h), and the queue's entry points.
#include <atomic>

#include "lo_ctx_def.h"

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
// The one place a pending hold leaves the host -- the oldest one, on the context stream.  The wait is bounded by
// pipe_bound, it gives up at once when the pipeline is broken, and a timeout marks the held scan's own DevState (its
// lane's) LO_ERR_PIPELINE.
static int pop_hold(lo_ctx* c) {
    ScanQueue& q = c->q;
    const ScanQueue::Hold h = q.holds[0];
    for (int i = 1; i < q.n_hold; ++i) q.holds[i - 1] = q.holds[i];
    if (--q.n_hold == 0) g_holding.fetch_sub(1, std::memory_order_relaxed);
    LO_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_wait_final, dim3(1), dim3(kWave), 0, c->stream, q.d_fin + kFinWords * h.lane, h.seq, h.st,
                       q.d_hbroken, q.pipe_bound);
    LO_HIP(c, hipGetLastError());
    return LO_OK;
}
// All pending holds, oldest first.  Called at the top of every entry point that enqueues on the context stream, reads
// from it, or changes what a queued scan reads (and by sync_all); a queue of scans places its holds by plan (apply_plan).
int flush_hold(lo_ctx* c) {
    while (c->q.n_hold > 0) {
        const int rc = pop_hold(c);
        if (rc != LO_OK) return rc;
    }
    return LO_OK;
}

// ---------------------------------------------------------------- snapshot, apply, emit
ScanPlanIn scan_snapshot(const lo_ctx* c, bool cand, bool timed, bool dev_count) {
    const ScanQueue& q = c->q;
    ScanPlanIn in{};
    in.depth = q.depth;
    in.depth_used = q.depth_used;
    in.depth_auto = q.depth_auto;
    in.others_holding = g_holding.load(std::memory_order_relaxed) - (q.n_hold > 0 ? 1 : 0);
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
        if (q.n_hold == 0) g_holding.fetch_add(1, std::memory_order_relaxed);
        q.holds[q.n_hold++] = ScanQueue::Hold{seq, lane, st};
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

int lo_scan_overlap_status(lo_ctx* c, long long out[2]) {
    if (!c || !out) return LO_ERR_ARG;
    out[0] = c->q.overlap ? 1 : 0;
    out[1] = static_cast<long long>(c->q.overlapped);
    return LO_OK;
}

}  // extern "C"
