// rt_assemble.h — the indexing of a shard's block and of the assembled frame
// (rt_export_shard*, rt_assemble*; DESIGN.md sections 17, 19 and 20), shared by
// the HIP kernels (rt_assemble.hip, device pass) and the CPU backend
// (rt_cpu.cpp, host pass).  Pure copies: no float operation, so the two
// backends agree bit for bit whatever their flags.
//
// rt_layout.h (rt_asm_args) has the block layout of the four plane counts and
// rt_block_shape_of, which says what a plane count holds.
//
// A pass is a list of items of VEC words (VEC = 4: 16 bytes, width % 4 == 0
// and every pointer 16-byte aligned; else VEC = 1), `slots` items per VEC
// pixels: slot k < 3 moves colour plane k, then the moment slot (blocks with
// moments) moves both moment planes — one float2 per pixel on the context's
// side, two planes on the block's — and the count slot (counted blocks) does
// the same for the pixels' uint2 {n_p, J_p}, moved as unsigned integers.
// Without moments the block has n_p alone: export moves only .x, assembly
// writes {n_p, 0} (no batch is tracked in a frame without moments).  Items are
// numbered slot-major, then row, then x, so consecutive items — a wave's lanes
// — write consecutive addresses and read one row segment.
#pragma once
#include "rt_path.h"

namespace {

template <class T>
struct AsmPair;
template <>
struct AsmPair<float> {
    typedef float2 two;
    typedef float4 four;
};
template <>
struct AsmPair<unsigned> {
    typedef uint2 two;
    typedef uint4 four;
};

// VEC words of T (float or unsigned), and VEC pixels' pairs {a, b} <-> VEC
// values of a and VEC values of b
template <class T, int VEC>
struct AsmWord {
    typedef T type;
    typedef typename AsmPair<T>::two pair;
    static RT_HD T fill(T v) { return v; }
    static RT_HD void split(const pair* p, T& a, T& b) {
        const pair t = p[0];
        a = t.x;
        b = t.y;
    }
    static RT_HD void join(pair* p, T a, T b) {
        pair t;
        t.x = a;
        t.y = b;
        p[0] = t;
    }
};
template <class T>
struct AsmWord<T, 4> {
    typedef typename AsmPair<T>::four type;
    typedef typename AsmPair<T>::two pair;
    static RT_HD type make(T x, T y, T z, T w) {
        type t;
        t.x = x;
        t.y = y;
        t.z = z;
        t.w = w;
        return t;
    }
    static RT_HD type fill(T v) { return make(v, v, v, v); }
    static RT_HD void split(const pair* p, type& a, type& b) {
        const type lo = reinterpret_cast<const type*>(p)[0], hi = reinterpret_cast<const type*>(p)[1];
        a = make(lo.x, lo.z, hi.x, hi.z);
        b = make(lo.y, lo.w, hi.y, hi.w);
    }
    static RT_HD void join(pair* p, type a, type b) {
        reinterpret_cast<type*>(p)[0] = make(a.x, b.x, a.y, b.y);
        reinterpret_cast<type*>(p)[1] = make(a.z, b.z, a.w, b.w);
    }
};

// items of a pass over `rows` rows of the block (export: rows_per_shard) or of
// the frame (assembly: height)
RT_HD long asm_items(const rt_asm_args& A, int rows, int vec) {
    return (long)rows * (A.width / vec) * rt_block_shape_of(A.planes).slots;
}

// The slot of item q, `per` items per slot: at most four slots, five of a
// counted block, so three or four compares instead of a 64-bit division; what
// is left of q fits 32 bits (a plane holds at most RT_ASM_MAX_PLANE words)
#define RT_ASM_MAX_PLANE (1ll << 31)
template <bool COUNTED>
RT_HD int asm_slot(long q, long per) {
    return (int)(q >= per) + (int)(q >= 2 * per) + (int)(q >= 3 * per) + (COUNTED ? (int)(q >= 4 * per) : 0);
}

// The item functions below take COUNTED = rt_block_shape_of(A.planes).counted
// as a template parameter: the passes of an uncounted block then carry nothing
// of the count slot (measured: DESIGN.md section 20).

// Export item q of rows_per_shard * (width / VEC) * slots: the context's
// frameSum (and moments, and counts) into its block; rows past the shard's are
// zero-filled.  A.cnt null: the accumulation is uniform, every pixel of the
// shard has the counts {A.n, A.j}
template <int VEC, bool COUNTED>
RT_HD void asm_export_item(const rt_asm_args& A, long q) {
    typedef AsmWord<float, VEC> F;
    typedef AsmWord<unsigned, VEC> U;
    typedef typename F::type word;
    typedef typename U::type cword;
    const rt_block_shape B = rt_block_shape_of(A.planes);
    const int wv = A.width / VEC;
    const long per = (long)A.rows_per_shard * wv;  // items (and words) of one block plane
    const int k = asm_slot<COUNTED>(q, per);
    // word (j, x) of the block plane, and of a shard plane: the same rows of width words
    const unsigned rem = (unsigned)(q - (long)k * per);
    const int j = (int)(rem / (unsigned)wv);
    const long npix = (long)A.rows * A.width;
    const bool count_slot = COUNTED && k >= 3 && !(B.moments && k == 3);
    const long at = (long)(count_slot ? B.count_plane : k) * per + rem;  // in the slot's first block plane
    if (k < 3) {
        word v = F::fill(0.0f);
        if (j < A.rows) v = reinterpret_cast<const word*>(A.sum + k * npix)[rem];
        (reinterpret_cast<word*>(A.block) + at)[0] = v;
    } else if (!count_slot) {
        word m = F::fill(0.0f), m2 = F::fill(0.0f);
        if (j < A.rows) F::split(A.mom + rem * VEC, m, m2);
        word* out = reinterpret_cast<word*>(A.block) + at;
        out[0] = m;
        out[per] = m2;
    } else {
        cword n = U::fill(0u), b = U::fill(0u);
        if (j < A.rows) {
            if (A.cnt) {
                U::split(A.cnt + rem * VEC, n, b);
            } else {
                n = U::fill(A.n);
                b = U::fill(A.j);
            }
        }
        cword* out = reinterpret_cast<cword*>(A.block) + at;
        out[0] = n;
        if (B.moments) out[per] = b;
    }
}

// Assembly item q of height * (width / VEC) * slots: row y of the frame from
// row y / shards of block y % shards.  Padding rows are never read.
template <int VEC, bool COUNTED>
RT_HD void asm_assemble_item(const rt_asm_args& A, long q) {
    typedef AsmWord<float, VEC> F;
    typedef AsmWord<unsigned, VEC> U;
    typedef typename F::type word;
    typedef typename U::type cword;
    const rt_block_shape B = rt_block_shape_of(A.planes);
    const int wv = A.width / VEC;
    const long per = (long)A.rows * wv;            // items (and words) of one frame plane
    const int k = asm_slot<COUNTED>(q, per);
    const unsigned rem = (unsigned)(q - (long)k * per);  // word (y, x) of the frame plane
    const int y = (int)(rem / (unsigned)wv);
    const int x = (int)(rem - (unsigned)y * (unsigned)wv);
    const int r = y % A.shards;
    const int j = y / A.shards;
    const long npix = (long)A.rows * A.width;
    const long bper = (long)A.rows_per_shard * wv;  // words of one block plane
    const bool count_slot = COUNTED && k >= 3 && !(B.moments && k == 3);
    const int plane = count_slot ? B.count_plane : k;  // the slot's first block plane
    const long at = (((long)r * A.planes + plane) * A.rows_per_shard + j) * wv + x;
    if (k < 3) {
        reinterpret_cast<word*>(A.sum + k * npix)[rem] = (reinterpret_cast<const word*>(A.block) + at)[0];
    } else if (!count_slot) {
        const word* in = reinterpret_cast<const word*>(A.block) + at;
        F::join(A.mom + rem * VEC, in[0], in[bper]);
    } else {
        const cword* in = reinterpret_cast<const cword*>(A.block) + at;
        U::join(A.cnt + rem * VEC, in[0], B.moments ? in[bper] : U::fill(0u));
    }
}

}  // namespace
