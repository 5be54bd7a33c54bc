"""lo::Buf (csrc/lo_buf.h), the owner of every device / pinned buffer, on the host alone.

A stand-alone C++ program instantiates the template with a fake allocator that counts calls and fails the k-th
allocation on request (LO_BUF_NO_HIP: no HIP runtime), and checks the contract the library relies on: a failed reserve
leaves the buffer empty, a grow frees the old block exactly once, a smaller reserve does nothing, moves empty their
source and free the destination's old block, and at the end every allocation was freed and no byte is counted live.
The program exits with the line number of the first check that fails.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lidar_odometry_amd", "csrc")

SOURCE = r"""
#define LO_BUF_NO_HIP
#include "lo_buf.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

static int n_alloc = 0, n_free = 0, fail_at = 0;   // fail_at: the allocation call (1-based, counted from now) that fails
static std::set<void*> live;                       // blocks handed out and not yet freed
static int double_free = 0;

static int fake_alloc(void** p, size_t bytes) {
    if (fail_at > 0 && --fail_at == 0) { *p = nullptr; return 2; }
    *p = std::malloc(bytes ? bytes : 1);
    live.insert(*p);
    ++n_alloc;
    return 0;
}
static void fake_free(void* p) {
    if (!live.erase(p)) ++double_free;
    else std::free(p);
    ++n_free;
}
template <class T> using TestBuf = lo::Buf<T, fake_alloc, fake_free>;

#define CHECK(x) do { if (!(x)) { std::printf("line %d: %s\n", __LINE__, #x); return __LINE__; } } while (0)
static long long bytes_live() { return lo::g_buf_live_bytes.load(); }

static int run() {
    {
        TestBuf<double> b;
        CHECK(b.get() == nullptr && b.capacity() == 0 && bytes_live() == 0);
        // a failed first reserve leaves it empty; the next one works
        fail_at = 1;
        CHECK(b.reserve(10) != 0);
        CHECK(b.get() == nullptr && b.capacity() == 0 && bytes_live() == 0 && n_alloc == 0 && n_free == 0);
        CHECK(b.reserve(10) == 0);
        CHECK(b.get() != nullptr && b.capacity() == 10 && bytes_live() == 80 && n_alloc == 1 && n_free == 0);
        // a smaller or equal count is a no-op
        double* const p10 = b.get();
        CHECK(b.reserve(4) == 0 && b.reserve(10) == 0 && b.reserve(0) == 0);
        CHECK(b.get() == p10 && b.capacity() == 10 && n_alloc == 1 && n_free == 0);
        // growing frees the old block exactly once, before the new one is allocated
        CHECK(b.reserve(100) == 0);
        CHECK(b.capacity() == 100 && n_alloc == 2 && n_free == 1 && live.size() == 1 && !live.count(p10));
        CHECK(bytes_live() == 800);
        // a failed grow: the old block is gone (freed once), no stale capacity, nothing counted live
        fail_at = 1;
        CHECK(b.reserve(1000) != 0);
        CHECK(b.get() == nullptr && b.capacity() == 0 && n_alloc == 2 && n_free == 2 && live.empty() && bytes_live() == 0);
        CHECK(b.reserve(5) == 0 && b.capacity() == 5 && bytes_live() == 40);
        // the pointer conversions the call sites use
        double* raw = b;
        CHECK(raw == b.get() && static_cast<bool>(b));
        b[4] = 1.5;
        CHECK(raw[4] == 1.5 && *(b + 4) == 1.5);

        // move construction empties the source
        TestBuf<double> c(std::move(b));
        CHECK(b.get() == nullptr && b.capacity() == 0 && c.get() == raw && c.capacity() == 5);
        CHECK(n_alloc == 3 && n_free == 2 && bytes_live() == 40);
        // move assignment frees the destination's old block and empties the source
        TestBuf<double> d;
        CHECK(d.reserve(7) == 0 && n_alloc == 4 && bytes_live() == 40 + 56);
        double* const p7 = d.get();
        d = std::move(c);
        CHECK(c.get() == nullptr && c.capacity() == 0 && d.get() == raw && d.capacity() == 5);
        CHECK(n_free == 3 && !live.count(p7) && live.count(raw) && bytes_live() == 40);
        // the moved-from buffers are usable again
        CHECK(c.reserve(3) == 0 && c.capacity() == 3 && bytes_live() == 40 + 24);
        // reset, and bytes of a void buffer
        d.reset();
        CHECK(d.get() == nullptr && d.capacity() == 0 && n_free == 4 && bytes_live() == 24);
        TestBuf<void> v;
        CHECK(v.reserve(33) == 0 && v.capacity() == 33 && bytes_live() == 24 + 33);
        struct Rec { int a, b; };
        TestBuf<Rec> r;
        CHECK(r.reserve(1) == 0);
        r->b = 7;
        CHECK(r.get()->b == 7);
    }   // c, v, r destroyed here
    CHECK(n_alloc == n_free && n_alloc == 7 && live.empty() && double_free == 0 && bytes_live() == 0);
    return 0;
}

int main() {
    const int rc = run();
    std::printf("%d allocations, %d frees, %lld bytes live\n", n_alloc, n_free, bytes_live());
    return rc == 0 ? 0 : 1;
}
"""


def test_buf_contract_with_a_counting_failing_allocator(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no host compiler")
    src = tmp_path / "buf_test.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "buf_test"
    p = subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "7 allocations, 7 frees, 0 bytes live", r.stdout
