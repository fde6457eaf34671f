// The ping-pong schedule with full-line A requests: the protocol and the geometry of the four default half / int8 matrix-core
// kernels, mfma_f16_pp2_kernel and mfma_f16_pp2s_kernel (mm_mfma_f16_kernels.inc), mfma_i8_pp2_kernel and mfma_i8_pp2s_kernel
// (mm_mfma_i8_kernels.inc).  DESIGN.md 3.18.
//
// The ping-pong schedule itself (two wave groups one barrier apart, the LDS-DMA hand-over rules) is described above GeoPP in
// mm_mfma_f16_kernels.inc.  With slabs of 64 bytes of k it gives A rows of 64 bytes, i.e. TWO L2 requests per 128-byte line
// (one per slab); measured: 817 M vs 546 M L2 requests per 16384^3 half launch at identical misses, on a kernel whose power
// budget goes into exactly that path.  Here A is staged in DOUBLE slabs [256 rows][128 B] (one request per
// line, chunk index ^ (row>>1)&7), each double slab serving two consecutive segments; B stays in slabs of 64 bytes of k per
// row of A ([32 k][512 B] half, [64 k][256 B] int8).  LDS: 3 A double slabs (96 KiB) + 4 B slabs (64 KiB) = all 160 KiB.  A
// wave still issues 4 DMA pieces per load segment: 2 of A (its half of double slab u/2 + 2) and 2 of B (slab u + 3); the
// counted vmcnt(8) and the barrier pairing are unchanged.  Requirements: K a multiple of two slabs and at least eight of them
// (half: K % 64 == 0, K >= 256; int8: K % 128 == 0, K >= 512).  The protocol is replayed on the CPU by
// tests/test_schedules.py, the LDS images and their swizzles by tests/test_layouts.py.
//
// What is here is what left every kernel's machine code as it was (profiles/pingpong2_isa_identity.txt): the geometry.  The
// four kernels still write the protocol out, each in its own body -- wave / lane decomposition, DMA offsets, issue lambdas, the
// segment, the seven-issue prologue, the 4-slab loop, the drain, the epilogue.  A kernel's body, moved unchanged into an
// always-inlined function template that the __global__ kernel calls, compiles to other code than it does as the kernel: the
// body is then optimised on its own before it is inlined and once more in the kernel, and the second pass does not leave it
// alone.  The same holds for the pieces (the epilogue, the two DMA issues).  A change to the protocol is made in all four, and
// in the replay of tests/test_schedules.py.
#pragma once

namespace mm {

// ES: bytes per operand element.  A slab is BK elements = 64 bytes of k deep; a B k-row is BROW = 256 * ES bytes.
template <int ES>
struct GeoPingPong2 {
  static constexpr int BM = 256, BN = 256, BK = 64 / ES, THREADS = 512;
  static constexpr int TM = 4, TN = 2;                            // the 32x32 forms: accumulators of a wavefront's 128 x 64 block
  static constexpr int A2_BYTES = BM * 128, NA = 3;               // A double slab: 32 KiB, ring of 3
  static constexpr int B_BYTES = BK * BN * ES, NB = 4;            // B slab: 16 KiB, ring of 4
  static constexpr int B_REGION = NA * A2_BYTES;
  static constexpr int LDS_BYTES = NA * A2_BYTES + NB * B_BYTES;  // 163840 = the whole LDS of a CU
  static constexpr int BROW = BN * ES;
};

}  // namespace mm
