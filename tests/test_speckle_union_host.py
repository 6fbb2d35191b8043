"""The union-find of DepthSpeckleFilter (csrc/kde_union.h) run on the host: a stand-alone program with its own main, built with
-fsanitize=address,undefined, calls the same uf_union text the kernels call from 16 std::threads on the seam lists of three
cases and compares the roots with a serial union-find.  The sanitisers are linked into that program only: nothing is
preloaded, nothing of it comes near Python or the GPU."""
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
