// wah_asm_blocks.hpp -- the hand-scheduled instruction blocks of the compress kernels, each written ONCE, as macros that
// expand to the string literal of an asm statement.  classify_pass1() / classify_pass2() (wah_compress.hip) and pair_pass2()
// (wah_compress_pair.inc) bind the operands; the statements there come in two or four parts because an asm statement
// takes at most 30 operands.
//
// A macro argument that names an operand (na, x3, m5 ...) is pasted into its %[...]; one that gives a group or step number
// is pasted into the text as an EXPRESSION (0 + 3, 8 + 1 ...), which the assembler evaluates: it picks the same
// inline-constant or literal encoding as for the plain number.  Labels carry the block-local number 0..7: %= is unique per
// asm statement.
#pragma once

#define WAH_STR_(a) #a
#define WAH_STR(a) WAH_STR_(a) // the argument's expansion, as text

// ===========================================================================
// compress_tile_body: a wavefront owns a segment, lane l of step s the group 64 s + l.
// Pass 1 needs nothing but the groups and leaves ONE register per segment behind; the kernel publishes the word counts of
// all its segments right after it and runs pass 2 while the other workgroups' counts are on their way.
//
// Operands: x0..x8 the groups of the half's steps and of the step after it (the one after step 15 = "never equal"),
// f the flag word (pass 1: bit 15 - s = step s; pass 2 expects it shifted to the top: bit 31 - s), na/ta and nb/tb two
// sets of temporaries (alternating between steps), cnt the scalar count, st a scalar temporary; pass 2: ps the packed
// position words, cn the running count in a VECTOR register (so that the ranking needs no scalar work), ln2 the lane id in
// both halves of a register, vb/pb LDS byte bases of the value / position arrays, dm the dump slot index (lanes that end
// no run store there: cheaper than masking EXEC).
// ===========================================================================

// PASS 1, eight steps (0-7 or 8-15, by the operands bound to it): which of the 64 groups of a step end a run.  The 64-lane
// mask of a step lives in VCC just long enough to be counted on the scalar unit (the sum = the words the segment
// compresses to) and to be shifted, lane by lane, into a per-lane flag word: v_addc_co f = f + f + vcc.  7 vector + 2
// scalar instructions per step, software-pipelined by one step so that every hazard slot (a DPP source must be two
// instructions old) is filled with the NEXT step's independent work.
//   carry and fill test of a step: its lane 0 into the temporary that the step before reads as "next group" in lane 63
#define WAH_P1_AHEAD(n, t, x, xn)                                                                                                       \
    "v_mov_b32_dpp %[" #n "], %[" #xn "] wave_rol:1 row_mask:0xf bank_mask:0xf\n\t"                                                    \
    "v_add_u32 %[" #t "], 1, %[" #x "]\n\t"                                                                                             \
    "v_and_b32 %[" #t "], 0x7ffffffe, %[" #t "]\n\t"
//   next group (lane 63 keeps the carry); z = (x ^ next) | t; run ends; FILL: the next step's WAH_P1_AHEAD or wait states;
//   f = 2 f + (this lane ends a run), which clobbers vcc
#define WAH_P1_STEP(n, t, x, FILL)                                                                                                      \
    "v_mov_b32_dpp %[" #n "], %[" #x "] wave_shl:1 row_mask:0xf bank_mask:0xf\n\t"                                                     \
    "v_bitop3_b32 %[" #n "], %[" #x "], %[" #n "], %[" #t "] bitop3:0xbe\n\t"                                                           \
    "v_cmp_ne_u32 vcc, 0, %[" #n "]\n\t"                                                                                                \
    FILL                                                                                                                                \
    "s_bcnt1_i32_b64 %[st], vcc\n\t"                                                                                                    \
    "v_addc_co_u32 %[f], vcc, %[f], %[f], vcc\n\t"                                                                                      \
    "s_add_u32 %[cnt], %[cnt], %[st]\n\t"
#define WAH_P1_BLOCK                                                                                                                    \
    WAH_P1_AHEAD(na, ta, x0, x1)                                                                                                        \
    WAH_P1_STEP(na, ta, x0, WAH_P1_AHEAD(nb, tb, x1, x2))                                                                               \
    WAH_P1_STEP(nb, tb, x1, WAH_P1_AHEAD(na, ta, x2, x3))                                                                               \
    WAH_P1_STEP(na, ta, x2, WAH_P1_AHEAD(nb, tb, x3, x4))                                                                               \
    WAH_P1_STEP(nb, tb, x3, WAH_P1_AHEAD(na, ta, x4, x5))                                                                               \
    WAH_P1_STEP(na, ta, x4, WAH_P1_AHEAD(nb, tb, x5, x6))                                                                               \
    WAH_P1_STEP(nb, tb, x5, WAH_P1_AHEAD(na, ta, x6, x7))                                                                               \
    WAH_P1_STEP(na, ta, x6, WAH_P1_AHEAD(nb, tb, x7, x8))                                                                               \
    WAH_P1_STEP(nb, tb, x7, "s_nop 1\n\t")

// PASS 2, steps s0 .. s0 + 7 (s0 = 0 | 8): the step's mask comes back out of the flag word (v_add_co f = f + f: the carry
// IS the mask), then the rank of every run end (v_mbcnt over the mask, seeded with the running count) and the compaction
// stores: the group's value at its rank, its position beside it.  8.5 vector + 2 LDS instructions per step.
// The mask of a step must be two instructions old before it is read as data: the address arithmetic and the stores of the
// step before fill those slots (in front of the first step: wait states).
#define WAH_P2_MASK "v_add_co_u32 %[f], vcc, %[f], %[f]\n\t" // vcc = the step's run ends (top bit of every lane's flag word)
//   POS: the position word, on even steps; non-end lanes: dump slot; NEXT: the next step's mask; ST: the position's store
#define WAH_P2_STEP(n, t, x, POS, NEXT, ST)                                                                                             \
    "v_mbcnt_lo_u32_b32 %[" #n "], vcc_lo, %[cn]\n\t"                                                                                   \
    "v_mbcnt_hi_u32_b32 %[" #n "], vcc_hi, %[" #n "]\n\t"                                                                               \
    "v_bcnt_u32_b32 %[cn], vcc_lo, %[cn]\n\t"                                                                                           \
    "v_bcnt_u32_b32 %[cn], vcc_hi, %[cn]\n\t"                                                                                           \
    POS                                                                                                                                 \
    "v_cndmask_b32 %[" #n "], %[dm], %[" #n "], vcc\n\t"                                                                                \
    NEXT                                                                                                                                \
    "v_lshl_add_u32 %[" #t "], %[" #n "], 2, %[vb]\n\t"                                                                                 \
    "v_lshl_add_u32 %[" #n "], %[" #n "], 1, %[pb]\n\t"                                                                                 \
    "ds_write_b32 %[" #t "], %[" #x "]\n\t"                                                                                             \
    ST " %[" #n "], %[ps]\n\t"
//   steps g (even) and g + 1: positions 64 g + lane and 64 (g + 1) + lane, packed; the odd step stores the high half
#define WAH_P2_TWO(xe, xo, g, LAST)                                                                                                     \
    WAH_P2_STEP(na, ta, xe, "v_add_u32 %[ps], ((64*((" WAH_STR(g) ")+1))<<16)|(64*(" WAH_STR(g) ")), %[ln2]\n\t", WAH_P2_MASK,          \
                "ds_write_b16")                                                                                                         \
    WAH_P2_STEP(nb, tb, xo, "", LAST, "ds_write_b16_d16_hi")
#define WAH_P2_BLOCK(s0)                                                                                                                \
    WAH_P2_MASK                                                                                                                         \
    "s_nop 1\n\t"                                                                                                                       \
    WAH_P2_TWO(x0, x1, s0 + 0, WAH_P2_MASK)                                                                                             \
    WAH_P2_TWO(x2, x3, s0 + 2, WAH_P2_MASK)                                                                                             \
    WAH_P2_TWO(x4, x5, s0 + 4, WAH_P2_MASK)                                                                                             \
    WAH_P2_TWO(x6, x7, s0 + 6, "")

// PASS 2 for a segment that compressed to few words (known from pass 1): a step without a single run end -- the inside of
// a long fill -- is branched over and costs one vector and two scalar instructions instead of eleven.  Nothing is
// pipelined across the branches, and every step builds its own position 64 g + lane in the low half (ln2: the lane id).
#define WAH_P2SKIP_STEP(n, t, j, g)                                                                                                     \
    WAH_P2_MASK                                                                                                                         \
    "s_cmp_eq_u64 vcc, 0\n\t"                                                                                                           \
    "s_cbranch_scc1 .Lwah_p2skip_%=_" #j "\n\t"                                                                                         \
    WAH_P2_STEP(n, t, x##j, "v_add_u32 %[ps], 64*(" WAH_STR(g) "), %[ln2]\n\t", "", "ds_write_b16")                                     \
    ".Lwah_p2skip_%=_" #j ":\n\t"
#define WAH_P2SKIP_BLOCK(s0)                                                                                                            \
    WAH_P2SKIP_STEP(na, ta, 0, s0 + 0)                                                                                                  \
    WAH_P2SKIP_STEP(nb, tb, 1, s0 + 1)                                                                                                  \
    WAH_P2SKIP_STEP(na, ta, 2, s0 + 2)                                                                                                  \
    WAH_P2SKIP_STEP(nb, tb, 3, s0 + 3)                                                                                                  \
    WAH_P2SKIP_STEP(na, ta, 4, s0 + 4)                                                                                                  \
    WAH_P2SKIP_STEP(nb, tb, 5, s0 + 5)                                                                                                  \
    WAH_P2SKIP_STEP(na, ta, 6, s0 + 6)                                                                                                  \
    WAH_P2SKIP_STEP(nb, tb, 7, s0 + 7)

// ===========================================================================
// compress_pair_kernel: a lane owns 32 CONSECUTIVE groups (= 31 words exactly), a wavefront two segments.
// PASS 2, groups k0 .. k0 + 7 (k0 = 0 | 8 | 16 | 24) of every lane: the lane's run-end flags come back out of its flag
// word one at a time (v_add_co f, mask, f, f: the carry is the 64-lane mask "lane ends a run at group k"), and the rest of
// the group's work runs under EXEC = that mask, so a lane that ends no run there keeps its registers without a single
// select:
//     word    = literal ? x : (x & 0x40000000) + (k + nl)                                              (kernels.cu:244-249)
//     LDS[ad] = word ; ad += 4 ; nl = 0x80000000 - k
// nl = 0x80000000 (the fill marker) minus the in-lane index of the lane's previous run end (in front of its first one: plus
// the distance to the last run end of the lanes below, from one DPP max-scan per pair), so k + nl is the fill marker plus
// the fill's length.
//
// Operands: x0..x7 the lane's groups, f the flag word (top bit = the block's first group), ad the LDS byte address of the
// lane's next word, nl (above), u / tb temporaries, m0..m7 the masks and sv the saved EXEC (scalar register pairs).
// ===========================================================================
#define WAH_PP2_MASK(j) "v_add_co_u32 %[f], %[m" #j "], %[f], %[f]\n\t"
//   the fill's type bit; 2 <= x + 1 (signed): neither 0 nor 0x7fffffff: a literal; fill word: type bit + (0x80000000 + length)
#define WAH_PP2_WORD(j, k)                                                                                                              \
    "s_mov_b64 exec, %[m" #j "]\n\t"                                                                                                    \
    "v_add_u32 %[u], 1, %[x" #j "]\n\t"                                                                                                 \
    "v_and_b32 %[tb], 0x40000000, %[x" #j "]\n\t"                                                                                       \
    "v_cmp_lt_i32 vcc, 1, %[u]\n\t"                                                                                                     \
    "v_add3_u32 %[tb], %[tb], %[nl], " WAH_STR(k) "\n\t"                                                                                \
    "v_mov_b32 %[nl], 0x80000000-(" WAH_STR(k) ")\n\t"                                                                                  \
    "v_cndmask_b32 %[tb], %[tb], %[x" #j "], vcc\n\t"
// skip, for pairs that compressed to few words: a group index at which NO lane ends a run is branched over: one vector and
// two scalar instructions.
#define WAH_PP2_GROUP_skip(j, k)                                                                                                        \
    "s_cmp_eq_u64 %[m" #j "], 0\n\t"                                                                                                    \
    "s_cbranch_scc1 .Lwah_pp2_%=_" #j "\n\t"                                                                                            \
    WAH_PP2_WORD(j, k)                                                                                                                  \
    "ds_write_b32 %[ad], %[tb]\n\t"                                                                                                     \
    "v_add_u32 %[ad], 4, %[ad]\n\t"                                                                                                     \
    ".Lwah_pp2_%=_" #j ":\n\t"
// swz: the same without the branches (8 vector + 1.25 scalar + 1 LDS instruction per group) and with the word stored at
// ad ^ ((ad >> 3) & 0x70): 16-byte piece c of the wave's 8 KB lives at piece c ^ ((c >> 3) & 7) (the layout of
// store_literals).  Lanes whose word counts are equal (32 in a stretch of literals, 16 in a periodic bitmap ...) would
// otherwise store to the same bank all at once.  Two more vector instructions per group; %[c70] = 0x70 in a scalar
// register (a VOP3 instruction takes no literal on this chip).
// (A third form -- neither branches nor swizzle -- served the pairs between the two thresholds of wah_compress_pair.inc;
// the thresholds are equal, kPairSparseBelow == kPairSwizzleFrom, and no pair reached it: removed.)
#define WAH_PP2_GROUP_swz(j, k)                                                                                                         \
    WAH_PP2_WORD(j, k)                                                                                                                  \
    "v_lshrrev_b32 %[u], 3, %[ad]\n\t"                                                                                                  \
    "v_bitop3_b32 %[u], %[ad], %[u], %[c70] bitop3:0x78\n\t" /* ad ^ (u & 0x70) */                                                      \
    "ds_write_b32 %[u], %[tb]\n\t"                                                                                                      \
    "v_add_u32 %[ad], 4, %[ad]\n\t"
// variant: skip | swz
#define WAH_PP2_BLOCK(variant, k0)                                                                                                      \
    "s_mov_b64 %[sv], exec\n\t"                                                                                                         \
    WAH_PP2_MASK(0) WAH_PP2_MASK(1) WAH_PP2_MASK(2) WAH_PP2_MASK(3) WAH_PP2_MASK(4) WAH_PP2_MASK(5) WAH_PP2_MASK(6) WAH_PP2_MASK(7)    \
    WAH_PP2_GROUP_##variant(0, k0 + 0)                                                                                                  \
    WAH_PP2_GROUP_##variant(1, k0 + 1)                                                                                                  \
    WAH_PP2_GROUP_##variant(2, k0 + 2)                                                                                                  \
    WAH_PP2_GROUP_##variant(3, k0 + 3)                                                                                                  \
    WAH_PP2_GROUP_##variant(4, k0 + 4)                                                                                                  \
    WAH_PP2_GROUP_##variant(5, k0 + 5)                                                                                                  \
    WAH_PP2_GROUP_##variant(6, k0 + 6)                                                                                                  \
    WAH_PP2_GROUP_##variant(7, k0 + 7)                                                                                                  \
    "s_mov_b64 exec, %[sv]\n\t"
