#!/usr/bin/env python3
"""Writes scan-rs_amd/csrc/tile_dense_body.inc: the round loop of the dense tile kernel (tiles_dense.inc, spmm_tile_dense_kernel)
as one hand-scheduled gfx950 instruction stream.

Why generated: the stream is unrolled over the 64 record positions of a round with four entry points, every register is a fixed
physical one (the accumulators are picked through VGPR index mode, which shifts EVERY vector destination while it is on, so no
compiler-scheduled instruction may sit between s_set_gpr_idx_on and _off), and LDS reads, scalar loads and LDS-DMA all have to
be counted by hand. A generator keeps the numbering honest; the output is committed next to it.

Register map (all clobbered by the asm statement; the compiler keeps v0-v25 and s0-s11; operands arrive in vector registers and are
read with v_readfirstlane_b32):
  v[88:215]   accumulators: slot q = v[88 + 4 q : 88 + 4 q + 3] (two f64: columns 2 lane, 2 lane + 1)
  v[56:87]    panel rows of 8 positions in flight (4 registers each)
  v[48:55]    their LDS addresses (v48 also: the offset of the records' "touch" load at the round's start)
  v[40:47]    weights of the round's 4 chunks: lane L holds weight L % 16 of the chunk (one register pair per chunk)
  v[38:39]    this lane's address in the weight stream: 8 (L % 16) behind the END of the NEXT round's weights
  v36 ring base of the lane (LDS address of its column pair in ring row 0), v37 row pitch in bytes
  v[26:33]    the NEXT round's weights as loaded: one register pair per chunk, lane L: weight L % 16 of the chunk (moved to v[40:47] at the
              round's start). v34 16 x lane: the lane's offset inside a 1 KB staging chunk (the chunk's own offset rides in the scalar base)
              (GEN_WDIRECT=0, the round's first form: v[26:27] next weights lane L = weight L, v[28:29] this round's, v30 the ds_bpermute
              address 4 x (lane % 16), v[31:35] the five staging chunks' offsets)
  (216 registers in all: two tile waves per SIMD leave 80 for a wave of the overflow gather, which runs beside this kernel)
  s[36:99]    the round's records: bits 7:0 = 4 x slot (the VGPR index), 15:8 = raw count (weight refresh only), 31:16 = ring row
  s[13:16]    copies of the last batch's four records (their chunk slot is reloaded before its FMAs)
  s17 wave << 10, s18 ring base, s19 ring end, s[20:21] END of the current round's records, s[22:23] round table,
  s[24:25] next tile to stage, s26 rounds left, s27 tile bytes, s31 tile bytes - 1024, s35 LDS address of the buffer staged into,
  s28 header of the current round (7:0 chunks, bit 8 = first round of a visit), s29 its chunk count, s34 / s101 / s12 the next
  three headers, s100 chunks of the next round, s30 / s[32:33] scratch (s[32:33]: where the next round's chunk slots come from)
  (stamp build: s[2:9] time stamps and sums, s[10:11] saved EXEC)

GEN_WSRC=tabo / tabi (round 6): the map is evaluated INSIDE the kernel - no weight stream. A position's weight is one entry of a table the
normalize refreshes (16 doubles per place of the layout when the outer side owns the map's nonlinear links, "tabo"; 16 planes over the
inner positions otherwise, "tabi"; entry 0 = 0.0 for null records, counts above 15 live in the overflow part), gathered by the
record's own (slot, count) or (ring row, count). Per round ONE vector load of the 64 records of the round after next (lane L = record
L of its four chunk slots; it also pulls them into L2 for the scalar loads, the stream form's "touch"), ONE 64-lane gather of the next
round's weights (lane L = weight of position L), and at the round's start the gathered register pair is spread into the form the
FMAs read (every row of 16 lanes = one chunk's 16 weights) by v_permlane16_swap / v_permlane32_swap (gfx950), no LDS involved:
  v[26:27]    the NEXT round's weights as gathered (lane L: position L); v28 the records of the round after next (lane L: record L)
  v[29:31]    address arithmetic; v32 tabi: 8 x plane stride; v33 4 x lane; v35 tabi: -1536 (one ring of 192 rows back, in bytes)
  v[38:39]    the table's base for this wave (tabo: the 32 places of its group; tabi: plane 0)
  s31         tabi: visit index of the current round (the staging code derives tile bytes - 1024 where it needs it)
"""
import os
import sys

PRIO = int(os.environ.get("GEN_PRIO") or 0)  # experiments (no gain, profiles/HISTORY.md): 1 = waves 4-7 at priority 1, 2 = two copies of the round whose priorities alternate per batch, opposite in the two waves of a SIMD
STAMP = bool(os.environ.get("GEN_STAMP"))  # diagnostic build: s_memtime stamps around the round's body, the staging wait and the barrier, summed per wave
SKIP = set((os.environ.get("GEN_SKIP") or "").split(","))  # timing experiments (wrong results): w = weights, r = records, b = barrier, d = staging, p = weight spreading (ds_bpermute)

PRE = (os.environ.get("GEN_PRE") or "0") != "0"  # experiment (slower by 0.3 ms per pass, profiles/HISTORY.md): the row reads of a round's first two batches are issued at the boundary in front of it (0: in the round's prologue)
WSRC = os.environ.get("GEN_WSRC") or "stream"  # where a position's weight comes from: stream = one f64 per position (pw, refreshed per normalize); tabo / tabi = gathered from the map's table by the record itself (see above)
TAB = WSRC in ("tabo", "tabi")
ALFIRST = (os.environ.get("GEN_ALFIRST") or "1") != "0"  # a round issues the row reads of its first two batches BEFORE it spreads its weights and starts the next round's loads: that work (45 instructions) then runs beside the reads' latency instead of in front of it - 0.5 ms per pass (round 6: 14.4 / 15.7 -> 13.9 / 15.2 on one box); 0: the round-5 order
ROTFIRST = (os.environ.get("GEN_ROTFIRST") or "0") != "0"  # experiment: the boundary's register rotation (and its wait for the next round's records) in FRONT of the visit's barrier instead of behind it
ONCE = (os.environ.get("GEN_ONCE") or "0") != "0"  # barrier form: a visit's tile is staged by its FIRST round only (the default re-stages it in every round of the visit so that one vmcnt count fits every boundary; a visit of more than 4 chunks then moves its 38 KB twice)
assert WSRC in ("stream", "tabo", "tabi")
WDIRECT = (os.environ.get("GEN_WDIRECT") or "1") != "0"  # a round's weights are loaded in the form the FMAs read (lane L: weight L % 16 of each chunk: four loads); 0: one load + eight ds_bpermute_b32
DMA_TOP = (os.environ.get("GEN_DMA") or "tail") == "top"  # staging loads at the round's start instead of in its last batches
BP = int(os.environ.get("GEN_BP") or 4)   # positions per batch (two batches of row reads in flight); 8 is as fast but takes 40 registers more
assert not TAB or (WDIRECT and not PRE and not DMA_TOP and BP == 4)
NB = 64 // BP     # batches per round
BPC = 16 // BP    # batches per chunk
ACC0 = 88
X0 = 56
A0 = 48
W0 = 40
R0 = 36


def xr(p, half):
    k = p % (2 * BP)
    b = X0 + 4 * k + 2 * half
    return f"v[{b}:{b + 1}]"


def xq(p):
    k = p % (2 * BP)
    return f"v[{X0 + 4 * k}:{X0 + 4 * k + 3}]"


def ad(p):
    return f"v{A0 + p % (2 * BP)}"


def rec(p):
    return f"s{R0 + p}"


def wreg(p):
    c = p // 16
    return f"v[{W0 + 2 * c}:{W0 + 2 * c + 1}]"


# timing experiment (wrong results): the positions p with p % 4 in SHARE do not read their panel row but use the row registers of the
# position in front of them - what the stream would cost if that share of the nonzeros found its row already in registers (a wave's
# nonzeros that name the same panel row: 61 % of them have such a partner at 32 cells x 3 %)
SHARE = {int(x) for x in (os.environ.get("GEN_SHARE") or "").split(",") if x}
RB = BP - len(SHARE)  # row reads per batch


def batch_AL(b, out):
    for j in range(BP):
        p = b * BP + j
        if j in SHARE:
            continue
        out.append(f"v_mad_u32_u16 {ad(p)}, {rec(p)}, v37, v36 op_sel:[1,0,0,0]")
    for j in range(BP):
        p = b * BP + j
        if j in SHARE:
            continue
        out.append(f"ds_read_b128 {xq(p)}, {ad(p)}")


def batch_F(b, out, tail=False):
    for j in range(BP):
        p = b * BP + j
        r = f"s{13 + j}" if tail else rec(p)
        if j == 0:
            out.append(f"s_set_gpr_idx_on {r}, 0x8")
        else:
            out.append(f"s_set_gpr_idx_idx {r}")
        q = p % 16
        ps = p - 1 if j in SHARE else p  # (experiment: the row of the position in front)
        out.append(f"v_fmac_f64_dpp v[{ACC0}:{ACC0 + 1}], {wreg(p)}, {xr(ps, 0)} row_newbcast:{q} row_mask:0xf bank_mask:0xf")
        out.append(f"v_fmac_f64_dpp v[{ACC0 + 2}:{ACC0 + 3}], {wreg(p)}, {xr(ps, 1)} row_newbcast:{q} row_mask:0xf bank_mask:0xf")
    out.append("s_set_gpr_idx_off")


def dma(i, out):
    """staging chunk i of the wave: LDS destination in M0 (one wait state before the LDS-DMA reads it), source = tile base + lane offset"""
    if "d" in SKIP:
        out.append("s_nop 0")
        return
    out.append(f"s_add_u32 s30, s17, {i * 8192}")
    if TAB:
        out.append("s_sub_u32 vcc_lo, s27, 0x400")
        out.append("s_min_u32 s30, s30, vcc_lo")
    else:
        out.append("s_min_u32 s30, s30, s31")
    out.append("s_add_u32 m0, s30, s35")
    if WDIRECT:
        # (the chunk's offset goes into the scalar base - VCC is free between two rounds' tops - and every chunk uses the one lane offset v34:
        # the five offset registers of the first form hold the next round's weights now)
        out.append("s_add_u32 vcc_lo, s24, s30")
        out.append("s_addc_u32 vcc_hi, s25, 0")
        out.append("global_load_lds_dwordx4 v34, vcc")
    else:
        out.append("s_nop 0")
        out.append(f"global_load_lds_dwordx4 v{31 + i}, s[24:25]")


def reload_slot(c, out):
    """records of chunk slot c for the NEXT round (s[32:33]: 256 bytes in front of its last record's end)"""
    out.append(f"s_load_dwordx16 s[{R0 + 16 * c}:{R0 + 16 * c + 15}], s[32:33], {hex(64 * c)}")


def tab_gather(out, next_round):
    """v[26:27] <- the table entries of the 64 records in v28 (lane L: record L of a round's four chunk slots).
    tabo: byte offset = slot x 128 + count x 8 inside the wave's 4 KB of the place table (16 doubles per place).
    tabi: entry = plane count, inner position = ring row + 192 q - (192 if the row's buffer index lies above m), with u' = visit - 1,
    q = u' / 4, m = u' % 4: the record's tile is the latest one at or below u' that sits in its ring buffer (the tiles a visit reads are
    u' and u' - 1). The compare works on the whole record (ring row = its upper half), row x 8 = record >> 13 (counts stay below 32).
    next_round: the visit is the NEXT round's (s31 + bit 8 of its header s34); else the current one (entry: round 0)."""
    a = out.append
    if WSRC == "tabo":
        a("v_and_b32 v30, 0xfc, v28")               # 4 x slot
        a("v_bfe_u32 v29, v28, 8, 8")               # count
        a("v_lshlrev_b32 v29, 3, v29")
        a("v_lshl_add_u32 v30, v30, 5, v29")        # slot x 128 + count x 8
    else:
        if next_round:
            a("s_bfe_u32 s30, s34, 0x10008")        # the next round opens a visit?
            a("s_add_u32 s30, s31, s30")
        else:
            a("s_mov_b32 s30, s31")
        a("s_max_u32 s30, s30, 1")
        a("s_sub_u32 s30, s30, 1")                  # u' (a part's first visit has no records: clamped)
        a("s_lshr_b32 m0, s30, 2")
        a("s_mul_i32 m0, m0, 0x600")                # 192 q rows, in bytes
        a("s_and_b32 s30, s30, 3")
        a("s_add_u32 s30, s30, 1")
        a("s_mul_i32 s30, s30, 0x300000")           # 48 (m + 1) << 16: first ring row of the buffers above m, as a record
        a("v_bfe_u32 v29, v28, 8, 8")               # count
        a("v_mul_lo_u32 v29, v29, v32")             # plane
        a("v_lshrrev_b32 v30, 13, v28")             # ring row x 8
        a("v_cmp_le_u32 vcc, s30, v28")
        a("v_cndmask_b32 v31, 0, v35, vcc")         # -1536: the buffer holds a tile of the ring's previous turn
        a("v_add3_u32 v30, v30, v29, v31")
        a("v_add_u32 v30, m0, v30")
    a("v_add_co_u32 v30, vcc, v38, v30")            # (address pairs are even-aligned on gfx90a and later)
    a("v_addc_co_u32 v31, vcc, 0, v39, vcc")
    a("global_load_dwordx2 v[26:27], v[30:31], off")


def tab_spread(out):
    """v[26:27] (lane L = weight of position L: row c of 16 lanes = chunk slot c) -> v[40 + 2 c : 41 + 2 c] = chunk c's row in all four
    rows. v_permlane16_swap a, b: a's odd rows <-> b's even rows; v_permlane32_swap a, b: a's upper half <-> b's lower half.
    [r0 r1 r2 r3] x 2 -> [r0 r0 r2 r2], [r1 r1 r3 r3] -> copies -> [r0 x 4], [r2 x 4], [r1 x 4], [r3 x 4]. A swap may not read a
    register a vector instruction wrote in the two instructions in front of it (check_swap_hazards)."""
    a = out.append
    w = lambda c, h: f"v{W0 + 2 * c + h}"
    for h in (0, 1):
        a(f"v_mov_b32 {w(0, h)}, v{26 + h}")
        a(f"v_mov_b32 {w(1, h)}, v{26 + h}")
    a(f"v_permlane16_swap_b32 {w(0, 0)}, {w(1, 0)}")
    a("s_nop 0")
    a(f"v_permlane16_swap_b32 {w(0, 1)}, {w(1, 1)}")
    for h in (0, 1):
        a(f"v_mov_b32 {w(2, h)}, {w(0, h)}")
        a(f"v_mov_b32 {w(3, h)}, {w(1, h)}")
    for h in (0, 1):
        a(f"v_permlane32_swap_b32 {w(0, h)}, {w(2, h)}")
        a(f"v_permlane32_swap_b32 {w(1, h)}, {w(3, h)}")


def gen():
    """One round = up to 4 chunks of 16 record positions, worked in batches of BP positions with two batches of row reads in flight.

    What is loaded when (everything for round r + 1 travels while round r computes; the boundary between two rounds waits for nothing
    that was not issued a good part of a round earlier):
      * records (64 scalar registers, chunk slot c = s[36 + 16 c ..]): slot c of the next round is reloaded as soon as this round has
        issued the last FMA that names it (behind F of batch 4 c + 3; slots the round does not enter: in its prologue; slot 3: in front
        of the last batch, whose four accumulator indices are copied to s[13:16] first). Scalar loads return out of order, so only the
        boundary's lgkmcnt(0) certifies them; the counted waits of the row reads in between stay correct (a count that includes scalar
        loads can only wait for MORE row reads than needed, one per scalar load still in flight);
      * weights: four 128-byte loads per round into v[26:33] (lane L: weight L % 16 of each of the four chunk slots that end at the next
        round's last one), moved to v[40:47] by eight v_mov at the next round's start (every row of 16 lanes then holds a chunk's 16
        weights, which v_fmac_f64_dpp row_newbcast picks from);
      * panel tiles: five LDS-DMA loads per wave and round, in the round's last four batches and behind it. A round that is not the
        first of its visit stages the same tile once more (same bytes, same place; nobody reads it before the visit after the next):
        with the same five loads in every round the boundary's vmcnt(5) means the same thing everywhere;
      * headers: three rounds ahead (s28 / s34 / s101 / s12)."""
    o = []
    a = o.append
    # ---- inputs into the fixed registers ----
    # (every operand arrives in a vector register: the compiler has a dozen scalar registers left beside this statement's)
    for name, lo in (("rec", 20), ("rtab", 22), ("src", 24)):
        a(f"v_readfirstlane_b32 s{lo}, %[{name}lo]")
        a(f"v_readfirstlane_b32 s{lo + 1}, %[{name}hi]")
    a("v_readfirstlane_b32 s26, %[nrounds]")  # (uniform values handed over in vector registers: the compiler has few scalar ones left for operands)
    a("v_readfirstlane_b32 s27, %[rowb]")
    a("s_mul_i32 s27, s27, 48")  # bytes of a tile of 48 rows
    if TAB:
        a("v_readfirstlane_b32 s31, %[t0]")  # first visit of the item (tabi: the visit counter); the ring buffer of its first tile follows from it
    else:
        a("v_readfirstlane_b32 s35, %[dst]")  # (uniform values handed over in vector registers: the compiler has few scalar ones left for operands)
    a("v_readfirstlane_b32 s17, %[wave10]")  # (uniform values handed over in vector registers: the compiler has few scalar ones left for operands)
    a("v_readfirstlane_b32 s18, %[lds0]")  # (uniform values handed over in vector registers: the compiler has few scalar ones left for operands)
    a("s_lshl_b32 s19, s27, 2")
    a("s_add_u32 s19, s19, s18")
    if TAB:
        a("s_and_b32 s30, s31, 3")
        a("s_mul_i32 s30, s30, s27")
        a("s_add_u32 s35, s18, s30")
        a("v_mov_b32 v38, %[tablo]")
        a("v_mov_b32 v39, %[tabhi]")
        a("v_mov_b32 v33, %[lane4]")
        if WSRC == "tabi":
            a("v_mov_b32 v32, %[stride8]")
            a("v_mov_b32 v35, 0xfffffa00")
    else:
        a("s_sub_u32 s31, s27, 0x400")
        a("v_mov_b32 v38, %[pwlo]")
        a("v_mov_b32 v39, %[pwhi]")
    a("v_mov_b32 v36, %[ring]")
    a("v_mov_b32 v37, %[rowb]")
    if WDIRECT:
        a("v_lshlrev_b32 v34, 2, %[lane4]")  # 16 x lane: the lane's offset inside a 1 KB staging chunk
    else:
        a("v_and_b32 v30, 60, %[lane4]")  # 4 (lane % 16): ds_bpermute address of this lane's weight inside a chunk
        a("v_lshlrev_b32 v28, 2, %[lane4]")  # 16 x lane (v28: free until the first round)
        for i in range(5):  # source offsets of the wave's five staging chunks: min((wave + 8 i) 1024, tile bytes - 1024) + 16 lane
            a(f"s_add_u32 s30, s17, {i * 8192}")
            a("s_min_u32 s30, s30, s31")
            a(f"v_add_u32 v{31 + i}, s30, v28")
    if PRIO == 1:
        a("s_cmp_ge_u32 s17, 0x1000")
        a("s_cbranch_scc0 LP0%=")
        a("s_setprio 1")
        a("LP0%=:")
    if STAMP:
        for r_ in (6, 7, 8, 9):
            a(f"s_mov_b32 s{r_}, 0")
    a("s_cmp_eq_u32 s26, 0")
    a("s_cbranch_scc1 LDONE%=")
    a("s_load_dwordx2 s[28:29], s[22:23], 0x0")  # headers of rounds 0 and 1
    a("s_load_dword s101, s[22:23], 0x8")        # ... 2
    a("s_waitcnt lgkmcnt(0)")
    a("s_mov_b32 s34, s29")
    a("s_and_b32 s29, s28, 0xff")                # chunks of round 0
    a("s_lshl_b32 s30, s29, 6")
    a("s_add_u32 s20, s20, s30")
    a("s_addc_u32 s21, s21, 0")
    a("s_sub_u32 s32, s20, 0x100")
    a("s_subb_u32 s33, s21, 0")
    for c in range(4):
        reload_slot(c, o)
    if TAB:
        a("global_load_dword v28, v33, s[32:33]")   # the records of round 0, lane L = record L of its four chunk slots
        a("s_waitcnt vmcnt(0)")
        tab_gather(o, next_round=False)             # weights of round 0
        a("s_and_b32 s100, s34, 0xff")
        a("s_lshl_b32 s30, s100, 6")
        a("s_add_u32 vcc_lo, s32, s30")
        a("s_addc_u32 vcc_hi, s33, 0")
        a("s_nop 3")                                # (a vector write of VCC five wait states in front of a vector-memory read of it)
        a("global_load_dword v28, v33, vcc")        # the records of round 1
    elif WDIRECT:
        a("s_lshl_b32 s30, s29, 7")
        a("v_add_co_u32 v38, vcc, s30, v38")
        a("v_addc_co_u32 v39, vcc, 0, v39, vcc")
        for c in range(4):
            a(f"global_load_dwordx2 v[{26 + 2 * c}:{27 + 2 * c}], v[38:39], off offset:{-512 + 128 * c}")  # weights of round 0
    else:
        a("s_lshl_b32 s30, s29, 7")
        a("v_add_co_u32 v38, vcc, s30, v38")
        a("v_addc_co_u32 v39, vcc, 0, v39, vcc")
        a("global_load_dwordx2 v[26:27], v[38:39], off offset:-512")  # weights of round 0
    a("s_waitcnt vmcnt(0) lgkmcnt(0)")           # ... and the item's first tile (staged by the caller)
    if not PRE:
        if "b" not in SKIP:
            a("s_barrier")                            # round 0 is the first of its visit
        a("s_add_u32 s24, s24, s27")
        a("s_addc_u32 s25, s25, 0")
        a("s_add_u32 s35, s35, s27")
        a("s_cmp_eq_u32 s35, s19")
        a("s_cselect_b32 s35, s18, s35")
    else:
        a("s_branch LENTER%=")                        # round 0 is the first of its visit: barrier, then its first row reads

    def advance():
        if "b" not in SKIP:
            a("s_barrier")
        a("s_add_u32 s24, s24, s27")
        a("s_addc_u32 s25, s25, 0")
        a("s_add_u32 s35, s35, s27")
        a("s_cmp_eq_u32 s35, s19")
        a("s_cselect_b32 s35, s18, s35")

    def top():
        """what a round starts for the rounds behind it: the next round's weights, the touch of the records two rounds ahead, the header three ahead"""
        a("s_and_b32 s100, s34, 0xff")               # chunks of the next round
        if TAB:
            a("s_lshl_b32 s30, s100, 6")                 # where the next round's four chunk slots come from
            a("s_add_u32 s32, s20, s30")
            a("s_addc_u32 s33, s21, 0")
            a("s_sub_u32 s32, s32, 0x100")
            a("s_subb_u32 s33, s33, 0")
            tab_gather(o, next_round=True)               # the next round's weights, by its records (loaded a round ago)
            a("s_and_b32 s30, s101, 0xff")               # ... and the records of the round after it: its four chunk slots end 64 x its chunks further on
            a("s_lshl_b32 s30, s30, 6")
            a("s_load_dword s12, s[22:23], 0xc")         # header three rounds ahead
            a("s_add_u32 vcc_lo, s32, s30")
            a("s_addc_u32 vcc_hi, s33, 0")
            a("global_load_dword v28, v33, vcc")         # (this load is also what pulls those records into L2 for their scalar loads: the stream form's touch)
            return
        a("s_lshl_b32 s30, s100, 7")
        a("v_add_co_u32 v38, vcc, s30, v38")         # behind the next round's weights
        a("v_addc_co_u32 v39, vcc, 0, v39, vcc")
        if "w" in SKIP:
            a("s_nop 0")
        elif WDIRECT:
            # lane L: weight L % 16 of each of the next round's four chunk slots (v[38:39] carries 8 (L % 16)): the form the FMAs' DPP
            # broadcast reads. Four loads of 128 distinct bytes each where one load + eight ds_bpermute_b32 stood: the permutes cost
            # 1.5 ms per pass (timing experiment GEN_SKIP=p), at the top of every round, in front of its first FMA
            for c in range(4):
                a(f"global_load_dwordx2 v[{26 + 2 * c}:{27 + 2 * c}], v[38:39], off offset:{-512 + 128 * c}")
        else:
            a("global_load_dwordx2 v[26:27], v[38:39], off offset:-512")
        a("s_lshl_b32 s30, s100, 6")                 # where the next round's four chunk slots come from
        a("s_add_u32 s32, s20, s30")
        a("s_addc_u32 s33, s21, 0")
        a("s_sub_u32 s32, s32, 0x100")
        a("s_subb_u32 s33, s33, 0")
        if "t" not in SKIP:
            # touch: the records of the round after the next one into L2 (their scalar loads, issued during the next round, then hit there:
            # without it a boundary waits for slot 3's load to come from HBM, +350 clk per round). An LDS-DMA load into 256 scratch bytes of
            # this wave behind the ring: it needs no register to land in, and it is this round's OLDEST vector-memory operation
            # (v48: an address register; an instruction reads its address operand at issue, so the row reads that named it are past it)
            if WDIRECT:
                a("v_lshrrev_b32 v48, 2, v34")       # 4 x lane: 256 bytes = four chunk slots
            else:
                a("s_min_u32 s30, s17, s31")
                a("v_sub_u32 v48, v31, s30")         # 16 x lane
                a("v_lshrrev_b32 v48, 2, v48")       # 4 x lane: 256 bytes = four chunk slots
            a("s_lshr_b32 s30, s17, 2")
            a("s_add_u32 s30, s30, s19")
            a("s_add_u32 m0, s30, 0x400")            # behind the ring and the row of zeros
            a("s_nop 0")
            a("global_load_lds_dword v48, s[32:33] offset:256")
        if DMA_TOP:
            for i_ in range(5):
                dma(i_, o)
        a("s_load_dword s12, s[22:23], 0xc")         # header three rounds ahead

    def spread_weights():
        if TAB:
            tab_spread(o)
            return
        if WDIRECT:
            for i_ in range(8):
                a(f"v_mov_b32 v{W0 + i_}, v{26 + i_}")   # (vector moves: more than the two wait states a DPP read of them needs lie before the first FMA)
            return
        a("v_mov_b32 v28, v26")
        a("v_mov_b32 v29, v27")
        if "p" in SKIP:  # timing experiment (wrong results): no spreading of the weights through ds_bpermute
            return
        for c in range(4):
            a(f"ds_bpermute_b32 v{W0 + 2 * c}, v30, v28 offset:{64 * c}")
            a(f"ds_bpermute_b32 v{W0 + 2 * c + 1}, v30, v29 offset:{64 * c}")

    def batches():
        for b in range(NB):
            a(f"LS{b}%=:")
            last = b == NB - 1
            a(f"s_waitcnt lgkmcnt({RB})" if not last else "s_waitcnt lgkmcnt(0)")
            if last:
                # the last batch names its accumulators through copies, so that slot 3 can be reloaded before its FMAs instead of behind them
                for j_ in range(BP):
                    a(f"s_mov_b32 s{13 + j_}, {rec(b * BP + j_)}")
                reload_slot(3, o)
                batch_F(b, o, tail=True)
            else:
                batch_F(b, o)
            if b % BPC == BPC - 1 and b // BPC < 3:
                reload_slot(b // BPC, o)
            if ONCE:
                if b == NB - 4:
                    a("s_bitcmp1_b32 s28, 8")
                    a("s_cbranch_scc0 LONCEX%=")
                    for i_ in range(5):
                        dma(i_, o)
                    a("LONCEX%=:")
            elif b >= NB - 4 and not DMA_TOP:
                dma(b - (NB - 4), o)
            if b + 2 < NB:
                batch_AL(b + 2, o)
        if not DMA_TOP and not ONCE:
            dma(4, o)

    def rotate():
        a("s_waitcnt lgkmcnt(0)")                    # the next round's records and the header
        if WSRC == "tabi":
            a("s_bfe_u32 s30, s34, 0x10008")         # the visit counter follows the round that becomes current
            a("s_add_u32 s31, s31, s30")
        a("s_mov_b32 s28, s34")
        a("s_mov_b32 s34, s101")
        a("s_mov_b32 s101, s12")
        a("s_add_u32 s22, s22, 4")
        a("s_addc_u32 s23, s23, 0")
        a("s_mov_b32 s29, s100")
        a("s_lshl_b32 s30, s100, 6")
        a("s_add_u32 s20, s20, s30")
        a("s_addc_u32 s21, s21, 0")

    def stamp_barrier_begin():
        if STAMP:
            a("s_memtime s[2:3]")

    def stamp_barrier_end():
        if STAMP:
            a("s_memtime s[4:5]")
            a("s_waitcnt lgkmcnt(0)")
            a("s_sub_u32 s10, s4, s2")
            a("s_add_u32 s8, s8, s10")   # barrier (with GEN_PRE the stamp's lgkmcnt(0) also waits for row reads in flight: an upper bound)

    if not PRE:
        # ---- one round (round-5 first form: everything a round needs is started at its top) ----
        a("LROUND%=:")
        if STAMP:
            a("s_memtime s[2:3]")
        if not ALFIRST:
            spread_weights()
            top()
        a("s_cmp_eq_u32 s29, 4")
        a("s_cbranch_scc1 LPRO0%=")
        a("s_cmp_eq_u32 s29, 3")
        a("s_cbranch_scc1 LPRO1%=")
        a("s_cmp_eq_u32 s29, 2")
        a("s_cbranch_scc1 LPRO2%=")
        a("s_cmp_eq_u32 s29, 1")
        a("s_cbranch_scc1 LPRO3%=")
        # an empty round (a visit nobody has work in yet: the first two of a part)
        if ALFIRST:
            spread_weights()
            top()
        for c in range(4):
            reload_slot(c, o)
        if not DMA_TOP:
            for i_ in range(5):
                dma(i_, o)
        a("s_branch LBND%=")
        # prologues: the slots this round does not enter, then the rows of its first two batches
        for c in (3, 2, 1, 0):
            a(f"LPRO{c}%=:")
            if not ALFIRST:
                for cc in range(c):
                    reload_slot(cc, o)
            batch_AL(BPC * c, o)
            batch_AL(BPC * c + 1, o)
            if ALFIRST:
                spread_weights()
                top()
                for cc in range(c):  # (behind top(): it says where the next round's slots come from)
                    reload_slot(cc, o)
            if c != 0 or ALFIRST:
                a(f"s_branch LS{BPC * c}%=")
        batches()
        # ---- boundary ----
        a("LBND%=:")
        if STAMP:
            a("s_memtime s[4:5]")
            a("s_waitcnt lgkmcnt(0)")
            a("s_sub_u32 s10, s4, s2")
            a("s_add_u32 s6, s6, s10")   # body
            a("s_add_u32 s9, s9, 1")     # rounds
        a("s_sub_u32 s26, s26, 1")
        a("s_cmp_eq_u32 s26, 0")
        a("s_cbranch_scc1 LDONE%=")
        if ONCE:
            a("s_bitcmp1_b32 s28, 8")                    # only a visit's first round has five staging loads behind the next round's weights
            a("s_cbranch_scc0 LV0%=")
            a("s_waitcnt vmcnt(5)")
            a("s_branch LV1%=")
            a("LV0%=:")
            a("s_waitcnt vmcnt(0)")
            a("LV1%=:")
        else:
            a("s_waitcnt vmcnt(5)")                      # the next round's weights; every staging load but this round's five
        if STAMP:
            a("s_memtime s[2:3]")
            a("s_waitcnt lgkmcnt(0)")
            a("s_sub_u32 s10, s2, s4")
            a("s_add_u32 s7, s7, s10")   # wait for vector memory (+ the scalar loads the stamp forces)
        if ROTFIRST:
            rotate()
            a("s_bitcmp1_b32 s28, 8")
            a("s_cbranch_scc0 LROUND%=")
            advance()
            stamp_barrier_end()
            a("s_branch LROUND%=")
        a("s_bitcmp1_b32 s34, 8")
        a("s_cbranch_scc0 LNB%=")
        advance()                                     # next round = first of a visit: the tile it reads first has landed for everybody, nobody reads the oldest one any more
        stamp_barrier_end()
        a("LNB%=:")
        rotate()
        a("s_branch LROUND%=")
    else:
        # ---- one round, second form: what the round needs FIRST is started at the boundary in front of it. Entering a round (LENTER:
        # its header in s28, its chunk count in s29, its records certified): weights into their rows; the loads for the rounds behind
        # it; the record slots it will not enter, reloaded; the row reads of its first two batches — in FRONT of the barrier when the
        # header says so (bit 9, set by the builder: none of those 8 positions names the tile that becomes readable behind this barrier
        # in any of the item's 8 waves), else behind it. The latency of those reads and the scalar work then run beside the barrier wait.
        a("LBATCH%=:")
        batches()
        a("LBND%=:")
        if STAMP:
            a("s_memtime s[4:5]")
            a("s_waitcnt lgkmcnt(0)")
            a("s_sub_u32 s10, s4, s2")
            a("s_add_u32 s6, s6, s10")   # body (from the end of the barrier)
            a("s_add_u32 s9, s9, 1")     # rounds
        a("s_sub_u32 s26, s26, 1")
        a("s_cmp_eq_u32 s26, 0")
        a("s_cbranch_scc1 LDONE%=")
        a("s_waitcnt vmcnt(5)")                      # the next round's weights; every staging load but this round's five
        if STAMP:
            a("s_memtime s[2:3]")
            a("s_waitcnt lgkmcnt(0)")
            a("s_sub_u32 s10, s2, s4")
            a("s_add_u32 s7, s7, s10")   # wait for vector memory
        rotate()
        a("LENTER%=:")
        spread_weights()
        top()
        a("s_cmp_eq_u32 s29, 0")
        a("s_cbranch_scc1 LEMPTY%=")
        a("s_bitcmp1_b32 s28, 8")                    # first round of a visit?
        a("s_cbranch_scc0 LPF%=")                    # no: no barrier
        a("s_bitcmp1_b32 s28, 9")                    # its first reads may go ahead of the barrier?
        a("s_cbranch_scc1 LPF%=")
        stamp_barrier_begin()
        advance()
        stamp_barrier_end()
        a("s_andn2_b32 s28, s28, 0x100")             # (the barrier is behind us)
        a("LPF%=:")
        for n, lab in ((4, 0), (3, 1), (2, 2)):
            a(f"s_cmp_eq_u32 s29, {n}")
            a(f"s_cbranch_scc1 LPF{lab}%=")
        for c in (3, 2, 1, 0):
            a(f"LPF{c}%=:")
            for cc in range(c):
                reload_slot(cc, o)
            batch_AL(BPC * c, o)
            batch_AL(BPC * c + 1, o)
            a("s_bitcmp1_b32 s28, 8")                # still a barrier to pass (reads went ahead of it)?
            a(f"s_cbranch_scc0 LS{BPC * c}%=")
            stamp_barrier_begin()
            advance()
            stamp_barrier_end()
            a(f"s_branch LS{BPC * c}%=")
        # an empty round (a visit nobody has work in yet: the first two of a part)
        a("LEMPTY%=:")
        a("s_bitcmp1_b32 s28, 8")
        a("s_cbranch_scc0 LEMPTY2%=")
        stamp_barrier_begin()
        advance()
        stamp_barrier_end()
        a("LEMPTY2%=:")
        for c in range(4):
            reload_slot(c, o)
        if not DMA_TOP:
            for i_ in range(5):
                dma(i_, o)
        a("s_branch LBND%=")
    a("LDONE%=:")
    if PRIO:
        a("s_setprio 0")
    a("s_waitcnt vmcnt(0) lgkmcnt(0)")           # nothing of this statement may land in a register later
    if STAMP:
        a("v_mov_b32 v30, 0")
        a("v_mov_b32 v29, 0")
        a("v_readfirstlane_b32 s2, %[stamplo]")
        a("v_readfirstlane_b32 s3, %[stamphi]")
        a("s_mov_b64 s[10:11], exec")
        a("s_mov_b64 exec, 1")  # one lane adds the wave's sums
        for i_, r_ in enumerate((6, 7, 8, 9)):
            a(f"v_mov_b32 v28, s{r_}")
            a(f"global_atomic_add_x2 v30, v[28:29], s[2:3] offset:{8 * i_}")
        # the barrier wait by wave number (8 more sums behind the four)
        a("s_lshr_b32 s12, s17, 7")  # 8 x wave
        a("v_mov_b32 v30, s12")
        a("v_mov_b32 v28, s8")
        a("global_atomic_add_x2 v30, v[28:29], s[2:3] offset:32")
        a("s_waitcnt vmcnt(0)")
        a("s_mov_b64 exec, s[10:11]")
    return o


def check_dpp_hazards(lines):
    """gfx950: a VALU write of a VGPR needs two wait states before a DPP instruction reads it, a VALU write of EXEC five. The compiler's
    hazard recognizer does not look into an asm statement, so the stream is checked here: the DPP sources of every
    v_fmac_f64_dpp (weights v40-v47: written by ds_bpermute_b32; rows v56-v87: written by ds_read_b128) must not be the destination
    of one of the two vector-ALU instructions in front of it, and no vector instruction may write EXEC at all."""
    import re

    def regs(tok):
        m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
        if m:
            return set(range(int(m.group(1)), int(m.group(2)) + 1))
        m = re.fullmatch(r"v(\d+)", tok)
        return {int(m.group(1))} if m else set()

    insts = [ln for ln in lines if not ln.endswith(":")]
    for i, ln in enumerate(insts):
        ops = [t.strip() for t in ln.split(None, 1)[1].split(",")] if " " in ln else []
        if ln.startswith("v_") and ops and ops[0].startswith("exec"):
            raise SystemExit(f"vector write of EXEC: {ln}")
        if not ln.startswith("v_fmac_f64_dpp"):
            continue
        src = regs(ops[1]) | regs(ops[2].split()[0])
        for back in (1, 2):
            if i - back < 0:
                break
            prev = insts[i - back]
            if not prev.startswith("v_") or prev.startswith("v_readfirstlane"):
                continue
            pops = [t.strip() for t in prev.split(None, 1)[1].split(",")]
            if regs(pops[0]) & src:
                raise SystemExit(f"DPP hazard: '{prev}' writes a source of '{ln}' {back} instruction(s) earlier")


def check_swap_hazards(lines):
    """gfx950: v_permlane16_swap_b32 / v_permlane32_swap_b32 read (and write) both operands; a vector-ALU write of either needs two wait
    states before the swap (the compiler puts s_nop 1 there; it does not look into an asm statement)."""
    import re

    insts = [ln for ln in lines if not ln.endswith(":")]
    for i, ln in enumerate(insts):
        if not ln.startswith("v_permlane"):
            continue
        ops = {t.strip() for t in ln.split(None, 1)[1].split(",")}
        states = 0
        for back in range(1, 4):
            if i - back < 0 or states >= 2:
                break
            prev = insts[i - back]
            m = re.fullmatch(r"s_nop (\d+)", prev)
            if prev.startswith("v_") and not prev.startswith("v_readfirstlane"):
                dst = {t.strip() for t in prev.split(None, 1)[1].split(",")[: 2 if prev.startswith("v_permlane") else 1]}
                if dst & ops:
                    raise SystemExit(f"swap hazard: '{prev}' writes an operand of '{ln}' {states} wait state(s) earlier")
            states += 1 + (int(m.group(1)) if m else 0)


def main():
    lines = gen()
    check_dpp_hazards(lines)
    check_swap_hazards(lines)
    here = os.path.dirname(os.path.abspath(__file__))
    name = "tile_dense_body.inc" if WSRC == "stream" else f"tile_dense_body_{WSRC}.inc"
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(here, "..", "scan-rs_amd", "csrc", name)
    with open(path, "w") as f:
        f.write("// generated by tools/gen_tile_dense_asm.py - do not edit\n")
        for ln in lines:
            f.write('"' + ln + '\\n"\n')
    print(f"{len(lines)} instructions / labels -> {os.path.normpath(path)}")


if __name__ == "__main__":
    main()
