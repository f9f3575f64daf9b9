// rt_assemble.h — the indexing of a shard's block and of the assembled frame
// (rt_export_shard, rt_assemble; counted blocks, section
// 19, at the end), shared by the HIP kernels (rt_assemble.hip, device pass) and
// the CPU backend (rt_cpu.cpp, host pass).  Pure copies: no float operation, so
// the two backends agree bit for bit whatever their flags.
//
// Block layout (rt_layout.h rt_asm_args, include/rt_abi.h): `planes` planes of
// rows_per_shard * width floats, plane k < 3 = plane k of frameSum, planes 3
// and 4 = M and M2; a plane holds the shard's rows in shard order, then zero
// rows up to rows_per_shard.  `gathered` is `shards` consecutive blocks, block
// r = rows r, r + shards, ...
//
// A pass is a list of items of VEC floats (VEC = 4: 16 bytes, width % 4 == 0
// and every pointer 16-byte aligned; else VEC = 1), `slots` items per VEC
// pixels: slot k < 3 moves colour plane k, slot 3 moves both moment planes (one
// float2 per pixel on the context's side, two planes on the block's).  Items
// are numbered slot-major, then row, then x, so consecutive items — a wave's
// lanes — write consecutive addresses and read one row segment.
#pragma once
#include "rt_path.h"

namespace {

template <int VEC>
struct AsmWord {
    typedef float type;
    static RT_HD float zero() { return 0.0f; }
    // VEC pixels' {M, M2} pairs <-> VEC values of M and VEC values of M2
    static RT_HD void split(const float2* p, float& m, float& m2) {
        const float2 t = p[0];
        m = t.x;
        m2 = t.y;
    }
    static RT_HD void join(float2* p, float m, float m2) { p[0] = make_float2(m, m2); }
};
template <>
struct AsmWord<4> {
    typedef float4 type;
    static RT_HD float4 zero() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
    static RT_HD void split(const float2* p, float4& m, float4& m2) {
        const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
        m = make_float4(a.x, a.z, b.x, b.z);
        m2 = make_float4(a.y, a.w, b.y, b.w);
    }
    static RT_HD void join(float2* p, float4 m, float4 m2) {
        reinterpret_cast<float4*>(p)[0] = make_float4(m.x, m2.x, m.y, m2.y);
        reinterpret_cast<float4*>(p)[1] = make_float4(m.z, m2.z, m.w, m2.w);
    }
};

// items of a pass over `rows` rows of the block (export: rows_per_shard) or of
// the frame (assembly: height)
RT_HD long asm_items(const rt_asm_args& A, int rows, int vec) {
    return (long)rows * (A.width / vec) * (A.planes == 5 ? 4 : 3);
}

// The slot of item q, `per` items per slot: at most four slots, so three
// compares instead of a 64-bit division; what is left of q fits 32 bits (a
// plane holds at most RT_ASM_MAX_PLANE words)
#define RT_ASM_MAX_PLANE (1ll << 31)
RT_HD int asm_slot(long q, long per) { return (int)(q >= per) + (int)(q >= 2 * per) + (int)(q >= 3 * per); }

// Export item q of rows_per_shard * (width / VEC) * slots: the context's
// frameSum (and moments) into its block; rows past the shard's are zero-filled
template <int VEC>
RT_HD void asm_export_item(const rt_asm_args& A, long q) {
    typedef typename AsmWord<VEC>::type word;
    const int wv = A.width / VEC;
    const long per = (long)A.rows_per_shard * wv;  // items (and words) of one block plane
    const int k = asm_slot(q, per);
    const unsigned rem = (unsigned)(q - (long)k * per);  // word (j, x) of the block plane
    const int j = (int)(rem / (unsigned)wv);
    const long npix = (long)A.rows * A.width;
    const long src = rem;                          // word (j, x) of a shard plane: the same rows of width words
    word* out = reinterpret_cast<word*>(A.block) + ((long)k * per + rem);
    if (k < 3) {
        word v = AsmWord<VEC>::zero();
        if (j < A.rows) v = reinterpret_cast<const word*>(A.sum + k * npix)[src];
        out[0] = v;
    } else {
        word m = AsmWord<VEC>::zero(), m2 = AsmWord<VEC>::zero();
        if (j < A.rows) AsmWord<VEC>::split(A.mom + src * VEC, m, m2);
        out[0] = m;
        out[per] = m2;
    }
}

// Assembly item q of height * (width / VEC) * slots: row y of the frame from
// row y / shards of block y % shards.  Padding rows are never read.
template <int VEC>
RT_HD void asm_assemble_item(const rt_asm_args& A, long q) {
    typedef typename AsmWord<VEC>::type word;
    const int wv = A.width / VEC;
    const long per = (long)A.rows * wv;            // items (and words) of one frame plane
    const int k = asm_slot(q, per);
    const unsigned rem = (unsigned)(q - (long)k * per);  // word (y, x) of the frame plane
    const int y = (int)(rem / (unsigned)wv);
    const int x = (int)(rem - (unsigned)y * (unsigned)wv);
    const int r = y % A.shards;
    const int j = y / A.shards;
    const long npix = (long)A.rows * A.width;
    const long bper = (long)A.rows_per_shard * wv;  // words of one block plane
    const word* in = reinterpret_cast<const word*>(A.block) + (((long)r * A.planes + k) * A.rows_per_shard + j) * wv + x;
    if (k < 3)
        reinterpret_cast<word*>(A.sum + k * npix)[rem] = in[0];
    else
        AsmWord<VEC>::join(A.mom + rem * VEC, in[0], in[bper]);
}

// ---- counted blocks (rt_layout.h rt_asmc_args) -----------
// The same passes with one more slot behind the colour (and moment) slots: the
// count slot, the moment slot's twin — one uint2 {n_p, J_p} per pixel on the
// context's side, the planes n_p and J_p on the block's.  With 4 planes the
// block has n_p alone: export moves only .x, assembly writes {n_p, 0} (no batch
// is tracked in a frame without moments).  The count words are moved as
// unsigned integers.

template <int VEC>
struct AsmCnt {
    typedef unsigned type;
    static RT_HD unsigned fill(unsigned v) { return v; }
    static RT_HD void split(const uint2* p, unsigned& n, unsigned& j) {
        const uint2 t = p[0];
        n = t.x;
        j = t.y;
    }
    static RT_HD void join(uint2* p, unsigned n, unsigned j) { p[0] = make_uint2(n, j); }
};
template <>
struct AsmCnt<4> {
    typedef uint4 type;
    static RT_HD uint4 fill(unsigned v) { return make_uint4(v, v, v, v); }
    static RT_HD void split(const uint2* p, uint4& n, uint4& j) {
        const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
        n = make_uint4(a.x, a.z, b.x, b.z);
        j = make_uint4(a.y, a.w, b.y, b.w);
    }
    static RT_HD void join(uint2* p, uint4 n, uint4 j) {
        reinterpret_cast<uint4*>(p)[0] = make_uint4(n.x, j.x, n.y, j.y);
        reinterpret_cast<uint4*>(p)[1] = make_uint4(n.z, j.z, n.w, j.w);
    }
};

RT_HD long asmc_items(const rt_asmc_args& C, int rows, int vec) {
    return (long)rows * (C.a.width / vec) * (C.a.planes == 7 ? 5 : 4);
}

// at most five slots: one compare more than asm_slot
RT_HD int asmc_slot(long q, long per) { return asm_slot(q, per) + (int)(q >= 4 * per); }

// Export item q of rows_per_shard * (width / VEC) * slots.  C.cnt null: the
// accumulation is uniform, every pixel of the shard has the counts {C.n, C.j}
template <int VEC>
RT_HD void asmc_export_item(const rt_asmc_args& C, long q) {
    typedef typename AsmWord<VEC>::type word;
    typedef typename AsmCnt<VEC>::type cword;
    const rt_asm_args& A = C.a;
    const int wv = A.width / VEC;
    const long per = (long)A.rows_per_shard * wv;  // items (and words) of one block plane
    const int k = asmc_slot(q, per);
    const unsigned rem = (unsigned)(q - (long)k * per);  // word (j, x) of the block plane
    const int j = (int)(rem / (unsigned)wv);
    const long npix = (long)A.rows * A.width;
    const bool moments = A.planes == 7;
    if (k < 3) {
        word v = AsmWord<VEC>::zero();
        if (j < A.rows) v = reinterpret_cast<const word*>(A.sum + k * npix)[rem];
        (reinterpret_cast<word*>(A.block) + ((long)k * per + rem))[0] = v;
    } else if (moments && k == 3) {
        word m = AsmWord<VEC>::zero(), m2 = AsmWord<VEC>::zero();
        if (j < A.rows) AsmWord<VEC>::split(A.mom + rem * VEC, m, m2);
        word* out = reinterpret_cast<word*>(A.block) + (3 * per + rem);
        out[0] = m;
        out[per] = m2;
    } else {  // the count slot: plane 3 (n_p alone), or planes 5 and 6
        cword n = AsmCnt<VEC>::fill(0u), b = AsmCnt<VEC>::fill(0u);
        if (j < A.rows) {
            if (C.cnt) {
                AsmCnt<VEC>::split(C.cnt + rem * VEC, n, b);
            } else {
                n = AsmCnt<VEC>::fill(C.n);
                b = AsmCnt<VEC>::fill(C.j);
            }
        }
        cword* out = reinterpret_cast<cword*>(A.block) + ((moments ? 5 : 3) * per + rem);
        out[0] = n;
        if (moments) out[per] = b;
    }
}

// Assembly item q of height * (width / VEC) * slots.  Padding rows are never read.
template <int VEC>
RT_HD void asmc_assemble_item(const rt_asmc_args& C, long q) {
    typedef typename AsmWord<VEC>::type word;
    typedef typename AsmCnt<VEC>::type cword;
    const rt_asm_args& A = C.a;
    const int wv = A.width / VEC;
    const long per = (long)A.rows * wv;            // items (and words) of one frame plane
    const int k = asmc_slot(q, per);
    const unsigned rem = (unsigned)(q - (long)k * per);  // word (y, x) of the frame plane
    const int y = (int)(rem / (unsigned)wv);
    const int x = (int)(rem - (unsigned)y * (unsigned)wv);
    const int r = y % A.shards;
    const int j = y / A.shards;
    const long npix = (long)A.rows * A.width;
    const long bper = (long)A.rows_per_shard * wv;  // words of one block plane
    const bool moments = A.planes == 7;
    const int plane = k < 3 || (moments && k == 3) ? k : moments ? 5 : 3;  // the slot's first block plane
    const long at = (((long)r * A.planes + plane) * A.rows_per_shard + j) * wv + x;
    if (k < 3) {
        reinterpret_cast<word*>(A.sum + k * npix)[rem] = (reinterpret_cast<const word*>(A.block) + at)[0];
    } else if (moments && k == 3) {
        const word* in = reinterpret_cast<const word*>(A.block) + at;
        AsmWord<VEC>::join(A.mom + rem * VEC, in[0], in[bper]);
    } else {
        const cword* in = reinterpret_cast<const cword*>(A.block) + at;
        AsmCnt<VEC>::join(C.cnt + rem * VEC, in[0], moments ? in[bper] : AsmCnt<VEC>::fill(0u));
    }
}

}  // namespace
