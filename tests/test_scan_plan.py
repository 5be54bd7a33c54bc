"""plan_scan (csrc/lo_scan_plan.h), the scan queue's decision for one scan, on the host alone.

A stand-alone C++ program includes the header (no HIP), simulates a queue -- it keeps the lane, the pending holds and
the depth they were placed for itself, and applies each plan the way enqueue_optimize does -- and checks the sequences
a queue of scans goes through at every depth and split (max_iterations = 4, candidates and pipeline on, nothing timed
unless said), then the queue's invariants over every prefix of a few thousand random settings and scans (fixed seed).
The program exits with the line number of the first check that fails.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_odometry_amd", "csrc")

SOURCE = r"""
#include "lo_scan_plan.h"

#include <cstdint>
#include <cstdio>

using namespace lo;

#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); return __LINE__; } } while (0)

// The queue as the library keeps it, and the settings and scan properties the snapshot carries.
struct Sim {
    ScanPlanIn in{};
    int hold_id[kMaxLanes] = {};   // the pending holds' scan numbers, oldest first (beside in.hold_lane)
    int next_id = 0;
    int last_out = -1;             // the last hold that left
    bool order_ok = true;          // holds left oldest first
    int popped[kMaxLanes] = {};    // the lanes of the holds the last scan put in front of its head
    int n_popped = 0;
    int head_clash = 0;            // heads placed on a lane that still had a hold pending

    Sim() {
        in.depth = in.depth_used = kDefaultDepth;
        in.depth_auto = true;
        in.pipe = in.overlap = true;
        in.pipe_main = 1;
        in.pipe_main_auto = true;
        in.cand = true;
        in.max_iterations = 4;
    }
    void pop() {
        if (hold_id[0] <= last_out) order_ok = false;
        last_out = hold_id[0];
        for (int i = 1; i < in.n_hold; ++i) { hold_id[i - 1] = hold_id[i]; in.hold_lane[i - 1] = in.hold_lane[i]; }
        --in.n_hold;
    }
    void flush() { while (in.n_hold > 0) pop(); }
    // the public setters flush first
    void set_depth(int d) { flush(); in.depth = d; in.depth_auto = false; }
    void set_split(int s) { flush(); in.pipe_main = s; in.pipe_main_auto = false; }
    // one scan: plan, then what enqueue_optimize does with it
    ScanPlan scan() {
        const ScanPlan p = plan_scan(in);
        const int id = next_id++;
        n_popped = 0;
        if (p.flush_before) flush();
        in.depth_used = p.depth;
        in.lane = p.lane;
        for (int i = 0; i < p.pops_before_head; ++i) { popped[n_popped++] = in.hold_lane[0]; pop(); }
        // the head goes here (depth 1: the one hold still pending is the previous scan's, on the lane just left)
        for (int i = 0; i < in.n_hold; ++i) if (in.hold_lane[i] == p.lane) ++head_clash;
        if (p.flush_after_head) flush();
        if (p.pipelined && p.push_hold) {
            in.hold_lane[in.n_hold] = p.lane;
            hold_id[in.n_hold++] = id;
        } else {
            flush();
        }
        return p;
    }
};

static int sequences() {
    {   // default: depth 4 auto, alone, no split chosen
        Sim q;
        for (int k = 0; k < 9; ++k) {
            const int held = q.in.n_hold;
            const ScanPlan p = q.scan();
            CHECK(p.depth == 4 && p.pipelined && p.push_hold && !p.flush_before && !p.flush_after_head);
            CHECK(p.lane == k % 4 && p.tail_stream == p.lane && p.overlaps == (k > 0));
            if (k == 0) CHECK(p.split == 2 && !p.signal_main && p.pops_before_head == 0 && p.tail_stream == 0);
            else CHECK(p.split == 0 && p.signal_main);
            if (k >= 1 && k <= 3) CHECK(p.pops_before_head == 0 && q.in.n_hold == held + 1);
            if (k >= 4) CHECK(p.pops_before_head == 1 && q.n_popped == 1 && q.popped[0] == k % 4 && held == 4);
        }
        CHECK(q.in.n_hold == 4 && q.order_ok && q.head_clash == 0);
    }
    {   // depth 1 chosen
        Sim q;
        q.set_depth(1);
        for (int k = 0; k < 7; ++k) {
            const ScanPlan p = q.scan();
            CHECK(p.depth == 1 && p.pipelined && p.push_hold && p.tail_stream == 0 && p.pops_before_head == 0);
            if (k == 0) CHECK(p.split == 2 && p.lane == 0 && !p.overlaps && !p.flush_after_head);
            else CHECK(p.split == 1 && p.lane == k % 2 && p.overlaps && p.flush_after_head && !p.flush_before);
            CHECK(!p.signal_main && q.in.n_hold == 1);
        }
        CHECK(q.order_ok && q.head_clash == 0);
    }
    {   // depth 2 chosen
        Sim q;
        q.set_depth(2);
        for (int k = 0; k < 7; ++k) {
            const ScanPlan p = q.scan();
            CHECK(p.depth == 2 && p.pipelined && p.push_hold && p.lane == k % 2 && p.tail_stream == p.lane);
            CHECK(p.split == (k == 0 ? 2 : 1) && !p.signal_main && !p.flush_after_head && !p.flush_before);
            CHECK(p.pops_before_head == (k >= 2 ? 1 : 0));
            if (k >= 2) CHECK(q.popped[0] == p.lane);
            CHECK(q.in.n_hold == (k == 0 ? 1 : 2));
        }
        CHECK(q.order_ok && q.head_clash == 0);
    }
    {   // depth 3 with an explicit split 1
        Sim q;
        q.set_depth(3);
        q.set_split(1);
        for (int k = 0; k < 8; ++k) {
            const ScanPlan p = q.scan();
            CHECK(p.depth == 3 && p.pipelined && p.push_hold && p.split == 1 && !p.signal_main);
            CHECK(p.lane == k % 3 && p.tail_stream == p.lane && p.pops_before_head == (k >= 3 ? 1 : 0));
            if (k >= 3) CHECK(q.popped[0] == p.lane);
        }
        CHECK(q.in.n_hold == 3 && q.order_ok && q.head_clash == 0);
    }
    {   // another context starts holding mid-queue, under auto depth
        Sim q;
        for (int k = 0; k < 3; ++k) q.scan();
        CHECK(q.in.n_hold == 3 && q.in.lane == 2);
        q.in.others_holding = 1;
        ScanPlan p = q.scan();
        CHECK(p.flush_before && p.depth == 1 && !p.overlaps && p.lane == 2 && p.split == 2 && p.pipelined && p.push_hold);
        CHECK(p.tail_stream == 0 && q.in.n_hold == 1 && q.in.depth_used == 1);
        p = q.scan();
        CHECK(!p.flush_before && p.depth == 1 && p.overlaps && p.split == 1 && p.flush_after_head && p.lane == 1);
        q.in.others_holding = 0;   // alone again: back to four in flight, behind a flush
        p = q.scan();
        CHECK(p.flush_before && p.depth == 4 && !p.overlaps && p.split == 2 && p.lane == 1);
        CHECK(q.order_ok && q.head_clash == 0);
    }
    for (int what = 0; what < 3; ++what) {   // a timed, a stage-timed and a device-counted scan, holds pending
        Sim q;
        for (int k = 0; k < 3; ++k) q.scan();
        q.in.timed = what == 0;
        q.in.stage_timing = what == 1;
        q.in.dev_count = what == 2;
        const ScanPlan p = q.scan();
        CHECK(p.flush_before && !p.overlaps && p.lane == 2 && p.pipelined && p.split == 2 && !p.push_hold);
        CHECK(p.pops_before_head == 0 && !p.flush_after_head && q.in.n_hold == 0);
    }
    for (int what = 0; what < 5; ++what) {   // scans that do not go down the pipeline
        Sim q;
        if (what == 4) q.set_split(2);
        for (int k = 0; k < 3; ++k) q.scan();
        CHECK(q.in.n_hold == 3);
        if (what == 0) q.in.kd = true;
        if (what == 1) q.in.cand = false;
        if (what == 2) q.in.pipe = false;
        if (what == 3) q.in.flagged = true;
        if (what == 4) q.in.max_iterations = 2;   // max_iterations <= split
        const ScanPlan p = q.scan();
        CHECK(!p.pipelined && !p.overlaps && p.flush_before && p.lane == 2 && !p.push_hold && q.in.n_hold == 0);
    }
    for (int depth = 2; depth <= 3; ++depth) {   // a queue that starts on lane 3, left by a depth-4 queue
        Sim q;
        for (int k = 0; k < 4; ++k) q.scan();
        CHECK(q.in.lane == 3);
        q.set_depth(depth);
        int lane = 3;
        for (int k = 0; k < 7; ++k) {
            const ScanPlan p = q.scan();
            if (k > 0) lane = (lane + 1) % depth;
            CHECK(p.lane == lane && p.pipelined && p.push_hold && p.overlaps == (k > 0) && q.in.n_hold <= depth);
        }
        CHECK(q.order_ok && q.head_clash == 0);
    }
    return 0;
}

static uint32_t rng_state = 12345u;
static uint32_t rnd(uint32_t n) {   // xorshift32
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5;
    return rng_state % n;
}

static int invariants() {
    Sim q;
    for (int step = 0; step < 6000; ++step) {
        const uint32_t r = rnd(16);
        if (r == 0) { q.set_depth(1 + static_cast<int>(rnd(kMaxLanes))); continue; }
        if (r == 1) { q.set_split(static_cast<int>(rnd(4))); continue; }
        if (r == 2) { q.flush(); q.in.overlap = rnd(4) != 0; continue; }
        if (r == 3) { q.flush(); q.in.pipe = rnd(4) != 0; continue; }
        if (r == 4) { q.flush(); continue; }                     // any other call of the library
        if (r == 5) q.in.others_holding = static_cast<int>(rnd(3));
        if (r == 6) { q.flush(); q.in.depth_auto = true; q.in.depth = kDefaultDepth; }
        q.in.timed = rnd(12) == 0;
        q.in.stage_timing = rnd(40) == 0;
        q.in.dev_count = rnd(12) == 0;
        q.in.cand = rnd(10) != 0;
        q.in.kd = rnd(40) == 0;
        q.in.flagged = rnd(60) == 0;
        q.in.max_iterations = 1 + static_cast<int>(rnd(5));
        const int held = q.in.n_hold;
        const ScanPlan p = q.scan();
        CHECK(q.in.n_hold <= p.depth && q.in.n_hold <= kMaxLanes);
        CHECK(q.order_ok);
        CHECK(q.head_clash == 0);
        CHECK(p.overlaps || q.in.n_hold <= 1);                   // nothing pending in front of a scan that does not overlap
        if (!p.overlaps) CHECK(p.flush_before == (held != 0) && p.pops_before_head == 0 && !p.flush_after_head);
        CHECK(p.pops_before_head <= held && p.lane >= 0 && p.lane < kMaxLanes && p.tail_stream >= 0 && p.tail_stream < kMaxLanes);
        CHECK(!p.push_hold || p.pipelined);
        CHECK(!p.overlaps || (p.pipelined && held > 0));
        if (q.in.flagged) { q.flush(); q.in.pipe = false; }      // the recovery: the pipeline off for this context
    }
    return 0;
}

int main() {
    int rc = sequences();
    if (rc == 0) rc = invariants();
    std::printf("%s\n", rc == 0 ? "scan plan ok" : "scan plan FAILED");
    return rc == 0 ? 0 : 1;
}
"""


def test_scan_plan_sequences_and_invariants(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host compiler")
    src = tmp_path / "scan_plan_test.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "scan_plan_test"
    p = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "scan plan ok", r.stdout
