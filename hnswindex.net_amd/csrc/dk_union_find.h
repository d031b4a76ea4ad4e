// dk_union_find.h -- the lock-free union-find over an int array on the device (ECL-CC's), shared by the component count of the graph
// mirror (dk_graph_info.h) and the duplicate groups of the flat scan (dk_exact.h).  No kernel lives
// here: two device functions and the atomics' order and scope.
#pragma once
#include <hip/hip_runtime.h>

namespace hnsw {

#define GI_RELAXED __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ---- the union-find of the component count (ECL-CC's): parent[v] <= v always, a root has parent[v] == v ------------------
// Every access to parent[] is a relaxed agent-scope atomic: a plain load could be hoisted out of the loops below.
// find: walks towards smaller ids, so it ends; on the way every node passed is pointed at its grandparent (path halving) with an
// atomic min -- the node is not a root (its parent differs from it, and a node never becomes a root again), and the new value is
// one of its ancestors, so parents only ever decrease.
__device__ __forceinline__ int uf_find(int *parent, int v)
{
    int p = __hip_atomic_load(parent + v, GI_RELAXED);
    while (p != v) {
        const int gp = __hip_atomic_load(parent + p, GI_RELAXED);
        if (gp != p) (void)__hip_atomic_fetch_min(parent + v, gp, GI_RELAXED);
        v = p;
        p = gp;
    }
    return v;
}
// union: the larger root is hooked under the smaller with a compare-exchange on the root itself, so only roots are hooked.  Where
// the exchange fails another lane has hooked that root in the meantime -- the forest has one root fewer -- and this lane goes on
// from the two nodes it had reached: it never waits for anyone, and there are at most n - 1 hooks in all.
__device__ __forceinline__ void uf_union(int *parent, int a, int b)
{
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        int expected = hi;
        if (__hip_atomic_compare_exchange_strong(parent + hi, &expected, lo, __ATOMIC_RELAXED, GI_RELAXED)) return;
    }
}

} // namespace hnsw
