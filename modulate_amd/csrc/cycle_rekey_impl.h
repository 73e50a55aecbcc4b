// cycle_rekey_impl.h -- device code of the rekey kernel (cycle_rekey_kernel.hip): the two-keystream block.  Included by that TU only
// and hashed with it (modgpu_rekey_kernel_source_hash).  The arithmetic is cycle_kernel_impl.h's ALG 2 (ks_word_carry), run for two
// keystreams at once; that header is included, not changed.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "cycle_kernel_impl.h"

namespace {

// ks_word2_carry's assembly block works in v[112:127] and s[94:95]: the rekey kernel's own allocation stays below them
#define MODGPU_REKEY_KEEP_OFF_THE_FIXED_TEMPORARIES __attribute__((amdgpu_num_vgpr(112), amdgpu_num_sgpr(94)))

// The keystream bytes of one 16-byte word under TWO keystreams whose first bytes have canonical states sa and sb: ks_word_carry's
// three instructions per byte (product mad, fold mad with the carry-out in VCC, one v_addc_co_u32_sdwa that canonicalises and packs)
// for each stream -- 30 mads and 15 addc per stream, 60 + 30 per block.  cycle_kernel_impl.h explains the arithmetic and why none
// of it can be said in C++; the constraints are the same, the registers are this block's own:
//   * product slots, three per stream rotating: v[112:117] for stream a, v[118:123] for stream b; folds: v[124:125] (a), v[126:127]
//     (b); s[94:95] takes the product mads' unused carry-out.  The rekey kernel carries amdgpu_num_vgpr(112) / amdgpu_num_sgpr(94)
//     so the register allocator cannot reach them; check_isa.py checks the ISA for it.
//   * VCC: one per wave, so the two streams' fold -> addc pairs take turns.  A VALU write of VCC needs 2 wait states before a VALU
//     reads it as carry-in: each fold is followed by its stream's product mad of the byte after next and one s_nop 0 (s_nop 1 for
//     the last two bytes, which have no product left to compute).
//   * SDWA dst_sel forwarding hazard (1 wait state before a VALU reads a partly written VGPR): the next addc of the same dword is
//     four instructions later, the other stream's instructions in between; the block ENDS with s_nop 0 for the compiler's first
//     reader of b3 (cycle_kernel_impl.h: its hazard recognizer does not look inside the block).
// a0 and b0 come in holding sa and sb (byte 0 of the word is the state itself); a1..a3, b1..b3 are written whole.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm" // "clobber list contains reserved registers: s94, s95" -- reserved by us, for this
__device__ __forceinline__ void ks_word2_carry(uint32_t sa, uint32_t sb, uint32_t (&wa)[4], uint32_t (&wb)[4])
{
    uint32_t zero = 0;
    uint64_t bias = 0x8000000000000000ull;
    asm("" : "+v"(zero), "+v"(bias)); // three VGPRs of constants
    const uint32_t m = lcg::M;
    uint32_t a0 = sa, a1, a2, a3, b0 = sb, b1, b2, b3;
#define M1A(P, Y) "v_mad_u64_u32 v[" P "], s[94:95], %[sa], %[" Y "], %[bias]\n\t"
#define M1B(P, Y) "v_mad_u64_u32 v[" P "], s[94:95], %[sb], %[" Y "], %[bias]\n\t"
#define M2A(PLO, P) "v_mad_u64_u32 v[124:125], vcc, v" PLO ", %[m], v[" P "]\n\t"
#define M2B(PLO, P) "v_mad_u64_u32 v[126:127], vcc, v" PLO ", %[m], v[" P "]\n\t"
#define NOP0 "s_nop 0\n\t"
#define NOP1 "s_nop 1\n\t"
#define ACA(W, SEL, UNUSED) "v_addc_co_u32_sdwa %[" W "], vcc, v125, %[zero], vcc dst_sel:BYTE_" SEL " dst_unused:" UNUSED " src0_sel:DWORD src1_sel:DWORD\n\t"
#define ACB(W, SEL, UNUSED) "v_addc_co_u32_sdwa %[" W "], vcc, v127, %[zero], vcc dst_sel:BYTE_" SEL " dst_unused:" UNUSED " src0_sel:DWORD src1_sel:DWORD\n\t"
    asm(
        M1A("112:113", "y1") M1B("118:119", "y1") M1A("114:115", "y2") M1B("120:121", "y2")
        M2A("112", "112:113") M1A("116:117", "y3") NOP0 ACA("a0", "1", "UNUSED_PRESERVE") M2B("118", "118:119") M1B("122:123", "y3") NOP0 ACB("b0", "1", "UNUSED_PRESERVE")
        M2A("114", "114:115") M1A("112:113", "y4") NOP0 ACA("a0", "2", "UNUSED_PRESERVE") M2B("120", "120:121") M1B("118:119", "y4") NOP0 ACB("b0", "2", "UNUSED_PRESERVE")
        M2A("116", "116:117") M1A("114:115", "y5") NOP0 ACA("a0", "3", "UNUSED_PRESERVE") M2B("122", "122:123") M1B("120:121", "y5") NOP0 ACB("b0", "3", "UNUSED_PRESERVE")
        M2A("112", "112:113") M1A("116:117", "y6") NOP0 ACA("a1", "0", "UNUSED_PAD") M2B("118", "118:119") M1B("122:123", "y6") NOP0 ACB("b1", "0", "UNUSED_PAD")
        M2A("114", "114:115") M1A("112:113", "y7") NOP0 ACA("a1", "1", "UNUSED_PRESERVE") M2B("120", "120:121") M1B("118:119", "y7") NOP0 ACB("b1", "1", "UNUSED_PRESERVE")
        M2A("116", "116:117") M1A("114:115", "y8") NOP0 ACA("a1", "2", "UNUSED_PRESERVE") M2B("122", "122:123") M1B("120:121", "y8") NOP0 ACB("b1", "2", "UNUSED_PRESERVE")
        M2A("112", "112:113") M1A("116:117", "y9") NOP0 ACA("a1", "3", "UNUSED_PRESERVE") M2B("118", "118:119") M1B("122:123", "y9") NOP0 ACB("b1", "3", "UNUSED_PRESERVE")
        M2A("114", "114:115") M1A("112:113", "y10") NOP0 ACA("a2", "0", "UNUSED_PAD") M2B("120", "120:121") M1B("118:119", "y10") NOP0 ACB("b2", "0", "UNUSED_PAD")
        M2A("116", "116:117") M1A("114:115", "y11") NOP0 ACA("a2", "1", "UNUSED_PRESERVE") M2B("122", "122:123") M1B("120:121", "y11") NOP0 ACB("b2", "1", "UNUSED_PRESERVE")
        M2A("112", "112:113") M1A("116:117", "y12") NOP0 ACA("a2", "2", "UNUSED_PRESERVE") M2B("118", "118:119") M1B("122:123", "y12") NOP0 ACB("b2", "2", "UNUSED_PRESERVE")
        M2A("114", "114:115") M1A("112:113", "y13") NOP0 ACA("a2", "3", "UNUSED_PRESERVE") M2B("120", "120:121") M1B("118:119", "y13") NOP0 ACB("b2", "3", "UNUSED_PRESERVE")
        M2A("116", "116:117") M1A("114:115", "y14") NOP0 ACA("a3", "0", "UNUSED_PAD") M2B("122", "122:123") M1B("120:121", "y14") NOP0 ACB("b3", "0", "UNUSED_PAD")
        M2A("112", "112:113") M1A("116:117", "y15") NOP0 ACA("a3", "1", "UNUSED_PRESERVE") M2B("118", "118:119") M1B("122:123", "y15") NOP0 ACB("b3", "1", "UNUSED_PRESERVE")
        M2A("114", "114:115") NOP1 ACA("a3", "2", "UNUSED_PRESERVE") M2B("120", "120:121") NOP1 ACB("b3", "2", "UNUSED_PRESERVE")
        M2A("116", "116:117") NOP1 ACA("a3", "3", "UNUSED_PRESERVE") M2B("122", "122:123") NOP1 ACB("b3", "3", "UNUSED_PRESERVE")
        NOP0 // (the wait state a consumer of b3 needs)
        : [a0] "+&v"(a0), [a1] "=&v"(a1), [a2] "=&v"(a2), [a3] "=&v"(a3), [b0] "+&v"(b0), [b1] "=&v"(b1), [b2] "=&v"(b2), [b3] "=&v"(b3)
        : [sa] "v"(sa), [sb] "v"(sb), [bias] "v"(bias), [zero] "v"(zero), [m] "s"(m),
          [y1] "s"(2u * lcg::kBytePow.v[1]), [y2] "s"(2u * lcg::kBytePow.v[2]), [y3] "s"(2u * lcg::kBytePow.v[3]), [y4] "s"(2u * lcg::kBytePow.v[4]),
          [y5] "s"(2u * lcg::kBytePow.v[5]), [y6] "s"(2u * lcg::kBytePow.v[6]), [y7] "s"(2u * lcg::kBytePow.v[7]), [y8] "s"(2u * lcg::kBytePow.v[8]),
          [y9] "s"(2u * lcg::kBytePow.v[9]), [y10] "s"(2u * lcg::kBytePow.v[10]), [y11] "s"(2u * lcg::kBytePow.v[11]), [y12] "s"(2u * lcg::kBytePow.v[12]),
          [y13] "s"(2u * lcg::kBytePow.v[13]), [y14] "s"(2u * lcg::kBytePow.v[14]), [y15] "s"(2u * lcg::kBytePow.v[15])
        : "v112", "v113", "v114", "v115", "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127",
          "s94", "s95", "vcc");
#undef M1A
#undef M1B
#undef M2A
#undef M2B
#undef NOP0
#undef NOP1
#undef ACA
#undef ACB
    wa[0] = a0;
    wa[1] = a1;
    wa[2] = a2;
    wa[3] = a3;
    wb[0] = b0;
    wb[1] = b1;
    wb[2] = b2;
    wb[3] = b3;
}
#pragma clang diagnostic pop

// x ^ y ^ z in one instruction.  gfx950 has no v_xor3_b32 (that is gfx10+); it has v_bitop3_b32, any function of three inputs given
// by its truth table, and 0x96 is the three-input XOR.  Said in assembly because clang selects two v_xor_b32 for the same C++
// (two issue slots instead of one).
__device__ __forceinline__ uint32_t xor3(uint32_t x, uint32_t y, uint32_t z)
{
    uint32_t r;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(x), "v"(y), "v"(z));
    return r;
}

// data ^ ks_a ^ ks_b for one 16-byte word.  Each keystream is the complement of its packed state bytes, and the two complements
// cancel: d ^ ~wa ^ ~wb = d ^ wa ^ wb, one three-input XOR (v_bitop3_b32 0x96) per dword.
__device__ __forceinline__ u32x4 rekey_word(u32x4 d, uint32_t sa, uint32_t sb)
{
    uint32_t wa[4], wb[4];
    ks_word2_carry(sa, sb, wa, wb);
    d.x = xor3(d.x, wa[0], wb[0]);
    d.y = xor3(d.y, wa[1], wb[1]);
    d.z = xor3(d.z, wa[2], wb[2]);
    d.w = xor3(d.w, wa[3], wb[3]);
    return d;
}

// One byte under both keystreams (head / tail bytes outside the aligned body): ~sa ^ ~sb = sa ^ sb.
__device__ __forceinline__ uint8_t rekey_byte(uint8_t d, uint32_t sa, uint32_t sb) { return (uint8_t)(d ^ (uint8_t)(sa ^ sb)); }

} // namespace
