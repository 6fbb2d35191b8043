// kde_union.h — the lock-free union-find of DepthSpeckleFilter (speckle_kernels.hip), as text that host code can call too:
// tests/test_speckle_union_host.py runs exactly these functions from 16 std::threads under the address and undefined-behaviour
// sanitisers.  Nothing here names a device: the memory is reached through an Ops object,
//     int load(int i)           any value cell i has ever held (a stale one is allowed)
//     int amin(int i, int v)    cell i becomes min(cell i, v) atomically; returns what it held before
// on a table in which cell i starts as i (a root holds itself).
//
// Why this is correct without any ordering between threads ("Depth speckle filter"): a cell only ever receives
// amin() with an index of its own component that is smaller than the cell's index, so (1) parents only decrease, (2) every
// value a cell has ever held lies in the cell's component and is <= its index, (3) a walk along loaded values strictly
// decreases and ends.  A union is done only when an amin() RETURNS the root it was aimed at -- at that instant the cell was
// still a root and now points into the other tree -- or when both walks end in the same cell.  Whatever else an amin()
// returns is the cell's true parent at that instant, and the link is carried on from there (old ~ hi was already true, so
// hi ~ lo is established by old ~ lo).  A stale load therefore costs an iteration and never a link; the roots at the end are
// the component minima.
//
// An amin() that REPLACES a parent old by a smaller v takes the link cell -> old out of the forest, so old ~ v has to hold
// without it.  The union carries exactly that on (above).  The walk shortens paths only where it holds already: it aims x at
// a value g that x's parent p has held (path halving).  p ~ g holds among the cells below x -- p held g --, and whatever x
// holds by then replaced p under this same rule, so it is joined to p, and through p to g, among the cells below x as well.
// (The first version aimed every cell it met at the root of its walk and went on along the parents those amin()s RETURNED:
// cells that were never on the walk.  Where such a cell's parent had fallen below that root it stopped, and the link it had
// just replaced was lost -- the randomised sweep found it, tests/speckle_cases.py `lost_link` keeps it.)
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KDE_UNION_FN __host__ __device__ inline
#else
#define KDE_UNION_FN inline
#endif

namespace kde {

// The hard cap of every loop below.  Structurally a walk ends after fewer steps than the cell's index and a union after
// fewer rounds than its larger root's index; the cap is what keeps a defect from hanging a kernel.  A caller that sees
// `capped` come back true counts it (kde_speckle_capped_*) and leaves.
constexpr int kUnionCap = 1 << 20;

// the root the walk from x ends in
template <class Ops>
KDE_UNION_FN int uf_find(Ops& m, int x, bool& capped)
{
    for (int i = 0; i < kUnionCap; i++) {
        const int p = m.load(x);
        if (p >= x) return x;                   // a root holds itself
        x = p;
    }
    capped = true;
    return x;
}

// the same, and every cell of the walk is aimed at a value its parent has held (path halving): amin() with a smaller index
// that is joined to the cell's parents without the link the amin() may replace
template <class Ops>
KDE_UNION_FN int uf_find_halve(Ops& m, int x, bool& capped)
{
    for (int i = 0; i < kUnionCap; i++) {
        const int p = m.load(x);
        if (p >= x) return x;                   // a root holds itself
        const int g = m.load(p);
        if (g >= p) return p;
        m.amin(x, g);
        x = p;
    }
    capped = true;
    return x;
}

// a ~ b
template <class Ops>
KDE_UNION_FN void uf_union(Ops& m, int a, int b, bool& capped)
{
    for (int i = 0; i < kUnionCap; i++) {
        a = uf_find_halve(m, a, capped);
        b = uf_find_halve(m, b, capped);
        if (capped || a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = m.amin(hi, lo);
        if (old == hi) return;                  // hi was a root until this amin: linked
        a = old;                                // hi had a parent already: old ~ hi, so old ~ lo is what remains
        b = lo;
    }
    capped = true;
}

}  // namespace kde
