"""The union-find of DepthSpeckleFilter (csrc/kde_union.h) run on the host: a stand-alone program with its own main, built with
-fsanitize=address,undefined, calls the same uf_union text the kernels call from 16 std::threads on the seam lists of three
cases and compares the roots with a serial union-find.  The sanitisers are linked into that program only: nothing is
preloaded, nothing of it comes near Python or the GPU.

A second program replays the unions of one tile (speckle_cases `lost_link`: S1's 228 threads with their 495 links) step by step:
every load and every atomic-min is one step, a seeded generator picks the thread that takes the next step, so a schedule is a
function of its number and every schedule is sequentially consistent.  With the header as it is no schedule loses a link; with
the first version of the walk (uf_find_compress, kept in that program as the text it was) schedule 241 and 24 others of the
first 8000 do -- the defect the randomised sweep of the depth stages met on the GPU, held here without one."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import speckle_cases as SC
from conftest import ROOT

CSRC = os.path.join(ROOT, "kinectdepthmapenhancement_amd", "csrc")

PROGRAM = r"""
#include "kde_union.h"

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

struct HostOps {
    std::atomic<int>* cell;
    int load(int i) const { return cell[i].load(std::memory_order_relaxed); }
    int amin(int i, int v) const
    {
        int old = cell[i].load(std::memory_order_relaxed);
        while (old > v && !cell[i].compare_exchange_weak(old, v, std::memory_order_relaxed)) {}
        return old;
    }
};

struct SerialOps {
    int* cell;
    int load(int i) const { return cell[i]; }
    int amin(int i, int v) const
    {
        const int old = cell[i];
        if (v < old) cell[i] = v;
        return old;
    }
};

// argv[1]: a file of "n m" and m pairs; 16 threads take the pairs round robin, each in another order
int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int n = 0, m = 0;
    if (std::fscanf(f, "%d %d", &n, &m) != 2 || n < 1 || m < 0) return 2;
    std::vector<int> a(m), b(m);
    for (int i = 0; i < m; i++)
        if (std::fscanf(f, "%d %d", &a[i], &b[i]) != 2 || a[i] < 0 || a[i] >= n || b[i] < 0 || b[i] >= n) return 2;
    std::fclose(f);
    std::vector<int> serial(n);
    for (int i = 0; i < n; i++) serial[i] = i;
    SerialOps so{serial.data()};
    bool capped = false;
    for (int i = 0; i < m; i++) kde::uf_union(so, a[i], b[i], capped);
    std::vector<std::atomic<int>> cells(n);
    for (int round = 0; round < 4; round++) {
        for (int i = 0; i < n; i++) cells[i].store(i);
        std::atomic<int> caps{0};
        std::vector<std::thread> threads;
        for (int t = 0; t < 16; t++)
            threads.emplace_back([&, t] {
                HostOps ho{cells.data()};
                bool c = false;
                // every pair twice, by two different threads, forwards and backwards: contention on the same roots
                for (int i = t; i < m; i += 16) kde::uf_union(ho, a[i], b[i], c);
                for (int i = m - 1 - ((t + round) % 16); i >= 0; i -= 16) kde::uf_union(ho, b[i], a[i], c);
                if (c) caps++;
            });
        for (auto& th : threads) th.join();
        if (caps.load()) {
            std::printf("capped %d\n", caps.load());
            return 1;
        }
        HostOps ho{cells.data()};
        for (int i = 0; i < n; i++) {
            const int want = kde::uf_find(so, i, capped), got = kde::uf_find(ho, i, capped);
            if (want != got || capped) {
                std::printf("cell %d: root %d, serial %d\n", i, got, want);
                return 1;
            }
        }
    }
    std::printf("ok %d %d\n", n, m);
    return 0;
}
"""


REPLAY = r"""
#include "kde_union.h"

#include <ucontext.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

// the first version of the walk, kept here as the text it was: the replay below loses a link with it
namespace first {
template <class Ops>
int uf_find_compress(Ops& m, int x, bool& capped)
{
    const int root = kde::uf_find(m, x, capped);
    for (int i = 0; i < kde::kUnionCap && x > root; i++) x = m.amin(x, root);
    return root;
}
template <class Ops>
void uf_union(Ops& m, int a, int b, bool& capped)
{
    for (int i = 0; i < kde::kUnionCap; i++) {
        a = uf_find_compress(m, a, capped);
        b = uf_find_compress(m, b, capped);
        if (capped || a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = m.amin(hi, lo);
        if (old == hi) return;
        a = old;
        b = lo;
    }
    capped = true;
}
}  // namespace first

static ucontext_t g_scheduler;
static ucontext_t* g_running = nullptr;

// every memory operation is one step of a schedule: the task hands over in front of it and performs it when it is resumed
struct StepOps {
    int* cell;
    int load(int i) const
    {
        swapcontext(g_running, &g_scheduler);
        return cell[i];
    }
    int amin(int i, int v) const
    {
        swapcontext(g_running, &g_scheduler);
        const int old = cell[i];
        if (v < old) cell[i] = v;
        return old;
    }
};
struct SerialOps {
    int* cell;
    int load(int i) const { return cell[i]; }
    int amin(int i, int v) const
    {
        const int old = cell[i];
        if (v < old) cell[i] = v;
        return old;
    }
};

struct Task {
    std::vector<int> a, b;
    ucontext_t ctx;
    std::vector<char> stack;
    bool done = false, capped = false;
};
static std::vector<Task> g_tasks;
static std::vector<int> g_cells;
static int g_version = 0;

static void run_task(int t)
{
    Task& k = g_tasks[t];
    StepOps ops{g_cells.data()};
    for (size_t i = 0; i < k.a.size(); i++) {
        if (g_version == 0) kde::uf_union(ops, k.a[i], k.b[i], k.capped);
        else first::uf_union(ops, k.a[i], k.b[i], k.capped);
    }
    k.done = true;
    swapcontext(&k.ctx, &g_scheduler);
}

// argv: pairs file ("n tasks", then per task "m" and m pairs), version (0: kde_union.h, 1: the first version), first schedule, schedules
int main(int argc, char** argv)
{
    if (argc != 5) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    g_version = std::atoi(argv[2]);
    const long first_schedule = std::atol(argv[3]), schedules = std::atol(argv[4]);
    int n = 0, tasks = 0;
    if (std::fscanf(f, "%d %d", &n, &tasks) != 2 || n < 1 || tasks < 1) return 2;
    g_tasks.resize(tasks);
    std::vector<int> serial(n);
    for (int i = 0; i < n; i++) serial[i] = i;
    SerialOps so{serial.data()};
    bool capped = false;
    for (Task& k : g_tasks) {
        int m = 0;
        if (std::fscanf(f, "%d", &m) != 1 || m < 1) return 2;
        k.a.resize(m);
        k.b.resize(m);
        for (int i = 0; i < m; i++) {
            if (std::fscanf(f, "%d %d", &k.a[i], &k.b[i]) != 2 || k.a[i] < 0 || k.a[i] >= n || k.b[i] < 0 || k.b[i] >= n) return 2;
            kde::uf_union(so, k.a[i], k.b[i], capped);
        }
        k.stack.resize(64 * 1024);
    }
    std::fclose(f);
    std::vector<int> want(n);
    for (int i = 0; i < n; i++) want[i] = kde::uf_find(so, i, capped);
    long lost = 0;
    g_cells.resize(n);
    for (long s = first_schedule; s < first_schedule + schedules; s++) {
        for (int i = 0; i < n; i++) g_cells[i] = i;
        std::vector<int> live(tasks);
        for (int t = 0; t < tasks; t++) {
            Task& k = g_tasks[t];
            k.done = k.capped = false;
            getcontext(&k.ctx);
            k.ctx.uc_stack.ss_sp = k.stack.data();
            k.ctx.uc_stack.ss_size = k.stack.size();
            k.ctx.uc_link = &g_scheduler;
            makecontext(&k.ctx, (void (*)())run_task, 1, t);
            live[t] = t;
        }
        uint64_t x = 0x9E3779B97F4A7C15ull * (uint64_t)(s + 1) + 1;     // xorshift64*: the schedule is a function of s alone
        while (!live.empty()) {
            x ^= x >> 12;
            x ^= x << 25;
            x ^= x >> 27;
            const size_t at = (size_t)(((x * 0x2545F4914F6CDD1Dull) >> 33) % live.size());
            Task& k = g_tasks[live[at]];
            g_running = &k.ctx;
            swapcontext(&g_scheduler, &k.ctx);
            if (k.done) {
                if (k.capped) return 3;
                live[at] = live.back();
                live.pop_back();
            }
        }
        SerialOps got{g_cells.data()};
        bool bad = false;
        for (int i = 0; i < n && !bad; i++) bad = kde::uf_find(got, i, capped) != want[i];
        if (bad) {
            lost++;
            std::printf("schedule %ld loses a link\n", s);
        }
    }
    std::printf("lost %ld of %ld\n", lost, schedules);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("union_host")
    src = d / "union_host.cpp"
    src.write_text(PROGRAM)
    exe = str(d / "union_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread", "-I", CSRC, "-o", exe, str(src)]
    # the runtime linked statically where the compiler has it (g++ links it dynamically by default): the program then starts
    # whatever else the loader brings in first
    r = subprocess.run(cmd + ["-static-libasan"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.timeout(600)
@pytest.mark.parametrize("name,conn", (("snake", 4), ("checker", 8), ("noise", 4)))
def test_sixteen_threads_find_the_serial_roots(program, tmp_path, name, conn):
    """the seam lists of the case (the pairs S2 unites, on top of the tile-local pairs, so that the walks are long), and the
    roots are the component minima of the statement"""
    p = SC.params(name, connectivity=conn)
    z = SC.sanitise(SC.depth_frames(name)[0], p["z_min"], p["z_max"])
    (sa, sb), (ta, tb) = SC.seam_pairs(z, p["max_diff"], p["rel_diff"], conn)
    assert sa.size > 0
    a, b = np.concatenate([ta, sa]), np.concatenate([tb, sb])
    path = tmp_path / "pairs.txt"
    with open(path, "w") as f:
        f.write(f"{z.size} {a.size}\n")
        f.write("\n".join(f"{int(i)} {int(j)}" for i, j in zip(a, b)))
    r = subprocess.run([program, str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.split() == ["ok", str(z.size), str(a.size)]
    # the serial answer the program compared with is the statement's
    lab = SC.components(z.size, a, b)
    want = SC.filter_parts(SC.depth_frames(name)[0], **dict(p, min_size=1))["all_labels"].reshape(-1)
    assert (lab[want >= 0] == want[want >= 0]).all()


@pytest.fixture(scope="module")
def replay(tmp_path_factory):
    """(the replay program, the file of the tile's threads and their links in S1's order: right, then down, rows ly and ly + 8)"""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    d = tmp_path_factory.mktemp("union_replay")
    src = d / "union_replay.cpp"
    src.write_text(REPLAY)
    exe = str(d / "union_replay")
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-I", CSRC, "-o", exe, str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    p = SC.params("lost_link")
    tile = SC.sanitise(SC.depth_frames("lost_link")[0][:SC.TILE[1], :SC.TILE[0]], p["z_min"], p["z_max"])
    right = SC.linked(tile[:, :-1], tile[:, 1:], p["max_diff"], p["rel_diff"])
    down = SC.linked(tile[:-1], tile[1:], p["max_diff"], p["rel_diff"])
    tasks = []
    for tid in range(256):
        lx, ly = tid & 31, tid >> 5
        pairs = []
        for row in (ly, ly + 8):
            cell = row * 32 + lx
            if lx < 31 and right[row, lx]:
                pairs.append((cell, cell + 1))
            if row < 15 and down[row, lx]:
                pairs.append((cell, cell + 32))
        if pairs:
            tasks.append(pairs)
    assert (len(tasks), sum(len(t) for t in tasks)) == (228, 495)
    path = d / "tile_links.txt"
    with open(path, "w") as f:
        f.write(f"{tile.size} {len(tasks)}\n")
        for pairs in tasks:
            f.write(f"{len(pairs)} " + " ".join(f"{a} {b}" for a, b in pairs) + "\n")
    return exe, str(path)


def _replay(replay, version, first, count):
    exe, path = replay
    r = subprocess.run([exe, path, str(version), str(first), str(count)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def test_no_schedule_of_the_tile_loses_a_link(replay):
    out = _replay(replay, 0, 0, 3000)
    assert out.strip().endswith("lost 0 of 3000"), out[-2000:]


def test_the_replay_finds_the_first_version_of_the_walk(replay):
    """the replay has teeth: the same schedules with the first version of the walk lose a link, among them schedule 241"""
    out = _replay(replay, 1, 0, 1000)
    assert "schedule 241 loses a link" in out and not out.strip().endswith("lost 0 of 1000"), out[-2000:]
    assert "loses" not in _replay(replay, 0, 241, 1)
