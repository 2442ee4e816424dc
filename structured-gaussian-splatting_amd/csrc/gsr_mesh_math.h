// gsr_mesh_math.h — connected components of a triangle mesh and the rule of mesh cleaning, per element, written
// once as GSR_HD inline functions: the kernels of gsr_mesh.hip call them on the device, tests/mesh_host.cpp compiles the same text
// with g++ and runs it from several threads under AddressSanitizer, UBSan and ThreadSanitizer.
//
// THE RULE.  A mesh is faces [F,3] int32 over V vertices.
//   valid face   its three indices lie in [0, V) and are pairwise different.  Any other face is invalid: it joins nothing, belongs to
//                no component and is always dropped.
//   connection   two valid faces are connected when they share a VERTEX (not an edge: sheets that touch in one point are one piece).
//   label        a component's label is the smallest vertex index it contains; labels [F] holds it per face, -1 for an invalid face.
//   sizes        sizes [V] holds at index `label` the number of faces of that component, 0 elsewhere.
//   threshold    a face is kept when it is valid and sizes[label] >= threshold (ties at the threshold are all kept).
//   kept vertex  a vertex is kept when a kept face names it.  Kept faces and kept vertices keep their relative order; faces are re-indexed.
//
// THE UNION-FIND.  parent [V] starts as parent[v] = v.  INVARIANT: parent[x] <= x always, and a parent only ever decreases.  Every
// write to parent after the start is a compare-and-swap of one of two kinds:
//   link   parent[hi]: hi -> lo with lo < hi, expected value hi: it succeeds only while hi is a root, at most once per word, ever;
//   halve  parent[x]: p -> g with g = parent[p] < p < x, expected value p: x is not a root and stays none.
// Both lower the word, so the invariant holds under any interleaving, and a value read from parent[x] at any time - a stale one too -
// is x itself or a smaller vertex of x's component.  Hence:
//   find   walks a strictly decreasing chain: it ends within x steps, whatever other lanes do meanwhile;
//   link   hangs the LARGER of two roots under the smaller.  A failed compare-and-swap returns parent[hi] < hi, and the search goes on
//          from there: every retry strictly lowers one of the two roots, and each failure is witnessed by the one successful link of
//          that word, so a lane tries at most V times;
//   result when all links are done the root of a component is a vertex that was never hung under a smaller one of its component: its
//          smallest index, whatever the interleaving.
// No lane ever waits for another lane.  Both loops are bounded all the same (MeshCaps): a bound that is hit sets the give-up word and
// the lane returns; outputs are then unspecified (never out of bounds), and the count call reports it.  The caps the library uses
// (mesh_caps) are the proven bounds above, so a give-up means that the invariant was broken from outside.
//
// Reads of parent inside find / link are relaxed atomic loads, not plain loads (a plain load in a loop may be kept in a register), and
// the atomics come through one small policy: the device's vector atomics in plain C++, the __atomic builtins on the host.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#ifndef GSR_HD
#if defined(__HIPCC__)
#define GSR_HD __host__ __device__ __forceinline__
#else
#define GSR_HD static inline
#endif
#endif

namespace gsr {

// ---- the atomics policy: relaxed everywhere (the algorithm needs atomicity of the single word, no ordering between words) ----------
GSR_HD int32_t mesh_atomic_load(const int32_t *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    return __atomic_load_n(p, __ATOMIC_RELAXED);
#endif
}

// -> the value the word held: `expected` when the swap took place
GSR_HD int32_t mesh_atomic_cas(int32_t *p, int32_t expected, int32_t desired)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(p, expected, desired);
#else
    __atomic_compare_exchange_n(p, &expected, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
    return expected;
#endif
}

GSR_HD void mesh_atomic_add(int32_t *p, int32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    __atomic_fetch_add(p, v, __ATOMIC_RELAXED);
#endif
}

// the give-up word: every lane that gives up stores the same 1
GSR_HD void mesh_give_up(uint32_t *word)
{
#if defined(__HIP_DEVICE_COMPILE__)
    *word = 1u;
#else
    __atomic_store_n(word, 1u, __ATOMIC_RELAXED);
#endif
}

// ---- the rule ---------------------------------------------------------------------------------------------------------------------
GSR_HD bool mesh_face_valid(int32_t a, int32_t b, int32_t c, int32_t V)
{
    return (uint32_t)a < (uint32_t)V && (uint32_t)b < (uint32_t)V && (uint32_t)c < (uint32_t)V && a != b && a != c && b != c;
}

// valid, label: the face's (label is read only for a valid face); sizes [V]
GSR_HD bool mesh_face_kept(bool valid, int32_t label, int32_t V, const int32_t *sizes, int32_t threshold)
{
    return valid && (uint32_t)label < (uint32_t)V && sizes[label] >= threshold;
}

// ---- the union-find ---------------------------------------------------------------------------------------------------------------
struct MeshCaps { uint32_t find_steps, link_tries; };

// the proven bounds: a chain below x has at most x < V links; a lane's link fails at most once per word
GSR_HD MeshCaps mesh_caps(int32_t V) { return MeshCaps{(uint32_t)V, (uint32_t)V}; }

// The root above x as far as this lane can see it, halving the path on the way.  0 <= x < V.
GSR_HD int32_t mesh_find(int32_t *parent, int32_t x, uint32_t max_steps, uint32_t *give_up)
{
    int32_t p = mesh_atomic_load(parent + x);
    for (uint32_t step = 0; p != x; ++step) {
        if (step >= max_steps || (uint32_t)p > (uint32_t)x) { mesh_give_up(give_up); return x; }      // (the second: the invariant, checked
                                                                                                      // before p is used as an index)
        const int32_t g = mesh_atomic_load(parent + p);
        if (g != p) mesh_atomic_cas(parent + x, p, g);          // halve: x skips p (lost to another lane: that one lowered it)
        x = p; p = g;
    }
    return x;
}

// a and b are in one component from now on.  0 <= a, b < V.
GSR_HD void mesh_link(int32_t *parent, int32_t a, int32_t b, MeshCaps caps, uint32_t *give_up)
{
    int32_t ra = mesh_find(parent, a, caps.find_steps, give_up), rb = mesh_find(parent, b, caps.find_steps, give_up);
    for (uint32_t tries = 0; ra != rb; ++tries) {
        if (tries >= caps.link_tries) { mesh_give_up(give_up); return; }
        const int32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
        const int32_t seen = mesh_atomic_cas(parent + hi, hi, lo);
        if (seen == hi) return;
        if ((uint32_t)seen > (uint32_t)hi) { mesh_give_up(give_up); return; }      // the invariant, checked before `seen` is an index
        ra = mesh_find(parent, seen, caps.find_steps, give_up);           // seen < hi: hi's new parent, set by another lane
        rb = lo;
    }
}

// one face of the link pass: (i0, i1) and (i0, i2); an invalid face joins nothing
GSR_HD void mesh_link_face(int32_t *parent, const int32_t *face, int32_t V, MeshCaps caps, uint32_t *give_up)
{
    const int32_t a = face[0], b = face[1], c = face[2];
    if (!mesh_face_valid(a, b, c, V)) return;
    mesh_link(parent, a, b, caps, give_up);
    mesh_link(parent, a, c, caps, give_up);
}

// one face of the label pass (all links are done): -> its label, the root above i0; -1 for an invalid face
GSR_HD int32_t mesh_face_root(int32_t *parent, const int32_t *face, int32_t V, uint32_t max_steps, uint32_t *give_up)
{
    const int32_t a = face[0], b = face[1], c = face[2];
    if (!mesh_face_valid(a, b, c, V)) return -1;
    return mesh_find(parent, a, max_steps, give_up);
}

// ... and counted in sizes, a face at a time (the host's form; k_mesh_label adds a wave's faces of one label with one atomicAdd -
// integer adds commute, so the sums are the same)
GSR_HD int32_t mesh_label_face(int32_t *parent, const int32_t *face, int32_t V, int32_t *sizes, uint32_t max_steps, uint32_t *give_up)
{
    const int32_t root = mesh_face_root(parent, face, V, max_steps, give_up);
    if (root >= 0) mesh_atomic_add(sizes + root, 1);
    return root;
}

}  // namespace gsr
