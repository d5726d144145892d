"""Generator of the implicit-GEMM convolution kernels (gfx950 assembly; conv2d_im2col.nim:42-88 without the im2col matrix):
f32_kernel.Gen's workgroup program -- A side, LDS ring, tile bodies, slice fold, epilogue -- with the B operand gathered from the NCHW
image through a tap table in LDS and, under Cfg.cpers, workgroups that walk units (image, tile) with pipelined transitions.  ConvGen
states B's registers where Gen.alloc asks for them and overrides what touches B or picks the tile; f32_kernel.make returns it for Cfg.conv."""
from .core import v, s, VCC, M0
from .f32_kernel import Gen, KA_SCHED, KA_SCHED2, KA_CONV0, KA_CONV1, KA_CONV2


class ConvGen(Gen):
    # ------------------------------------------------------------------ registers
    STB_REGS, HAS_VVB, C_STRIDED = 2, False, False

    def alloc_sched(self):
        """one tile per workgroup (the GEMM scheduler's state would not fit beside the tap arithmetic: the kernels are out of SGPRs);
        its constants alias the tap scratch (alloc_WB)"""
        assert not self.c.persistent
        self.s_Keff, self.s_tile = self.s_K, None
        if self.c.cpers:
            self.s_tcur, self.s_img = self.p.salloc(), self.p.salloc()   # the next unit of this workgroup; the image of the tile being loaded

    def alloc_WB(self):
        S, V = self.p.salloc, self.p.valloc
        self.WB = [[self.triple(False) for _ in range(2)] for _ in range(4)]       # [pair][pixel of the piece][stage]
        self.vB0 = [V() for _ in range(8)]             # per piece: buffer offset of the lane's first / second pixel for the
        self.vB1 = [V() for _ in range(8)]             # piece's tap (read from the LDS table; 0x80000000 = padding)
        scr = S(16, align=4)
        self.s_scr = scr
        self.s_koff = [scr[i] for i in range(8)]       # per piece: (c*H*W + kh*W + kw) * 4 of the k it gathers
        self.s_k0 = S()                                # this wave's first k (= c * taps + kh * kW + kw) in the tile being loaded
        self.s_NT, self.s_kW, self.s_M10 = S(), S(), S()   # taps kH * kW; kW; ceil(1024 / kW): r / kW = (r * M10) >> 10 for r < 49
        self.s_pok = [S(2), S(2)]                      # prologue: lanes whose first / second output pixel exists (ragged last tile)
        self.s_m = S(2)
        self.s_HW4, self.s_W4, self.s_Cin = S(), S(), S()
        self.s_sc = scr.sub(0, 8)                      # (the scheduler constants are dead before conv_setup loads the geometry)

    def alloc_epi(self):     # (out of SGPRs: the tap state is dead by the epilogue)
        self.srdBias, self.s_epi = self.s_scr.sub(0, 4), self.s_scr.sub(4, 4)

    # ------------------------------------------------------------------ prologue
    def prologue(self):
        """Gen.prologue for a workgroup with one tile of image `workgroup id y`, or (Cfg.cpers) the units it walks"""
        c, p, e = self.c, self.p, self.p.emit
        self.once()
        self.L_run, self.L_exit = p.label("next_run"), p.label("exit")
        self.L_setup, self.L_recv = p.label("setup"), p.label("recv")
        if c.cpers:
            e("s_mov_b32", self.s_tcur, s(2))
            p.place(self.L_run)
            e("s_barrier", comment="every wave is done with the previous unit's LDS tiles and tap table")
            self.next_unit(self.L_exit)
        else:
            self.tile_origin(self.wg_tile())      # (no tile base: KA_TAB's low word is the taps' magic number here)
        self.run_setup()

    def batch_offsets(self, ka_bsa):
        pass      # (the image index moves B and C: conv_setup, c_base)

    def xpieces_B(self):
        pass      # (per tile: conv_setup)

    def b_descriptor(self, again=False):
        self.conv_setup(again)
        if self.c.debug:
            for r_ in range(0, 20, 4):
                self.dump_lds(f"tab[{r_ * 256}+4tid]", r_ * 256)
            self.dump("conv k0", self.s_k0)
            self.dump("conv HW4", self.s_HW4)
            self.dump("conv Cin", self.s_Cin)
            self.dump("conv WB00", self.lds_at(self.WB[0][0][2])[0])
            self.dump("conv WB31", self.lds_at(self.WB[3][1][2])[0])
        self.p.emit("s_mov_b32", self.srdB[3], 0x00020000)

    def dump_stB(self):
        super().dump_stB()
        for i_ in range(8):
            self.dump(f"conv koff[{i_}]", self.s_koff[i_])
            self.dump(f"conv vB0[{i_}]", self.vB0[i_])
            self.dump(f"conv vB1[{i_}]", self.vB1[i_])
            self.dump(f"conv stB[{i_}][0]", self.stB[i_][0])
            self.dump(f"conv stB[{i_}][1]", self.stB[i_][1])

    def store_tile0_early(self):
        # (the gathers of a tile are requested before its filter pieces: stored in that order, so that every counted wait names
        # tile 0's loads; the table reads of tile 1's gathers were waited for before these stores were issued, in the other path
        # after them: all LDS operations drained here keeps the two paths' queues alike)
        self.run_ops([o for grp in self.conv_store_ops(2) for o in grp])
        for pi in range(self.c.NPA):
            self.store_A_piece(pi, k=2)
        self.lg_wait(None)

    def store_tile_to_lds(self, k):
        for pi in range(self.c.NPA):
            self.store_A_piece(pi, k=k)
        self.run_ops([o for grp in self.conv_store_ops(k) for o in grp])

    def c_base(self, C_):
        """C's base is the image's [M][oH*oW] block"""
        e, st = self.p.emit, self.s_t
        img = self.s_img if self.c.cpers else s(3)
        e("s_mul_hi_u32", st[2], img, self.s_scr[12])
        e("s_mul_i32", st[0], img, self.s_scr[12])
        e("s_add_u32", self.srdC[0], C_[0], st[0])
        e("s_addc_u32", self.srdC[1], C_[1], st[2])
        e("s_and_b32", self.srdC[1], self.srdC[1], 0xffff)

    def issue_loads_all(self):      # (B's gathers first, like the loop body: the two queues must carry the same order)
        self.run_ops([o for grp in self.conv_load_ops() for o in grp])
        for pi in range(self.c.NPA):
            self.load_A_piece(pi)

    def k_steps(self):
        return super().k_steps()[:1]      # (A only: B's k rides in the gathers' scalar offsets)

    def mask_last_pieces_if(self, sreg, value):
        pass      # (the launcher pads the filter's rows to whole pieces; B's k beyond K selects the table's "nothing" entry)

    # ------------------------------------------------------------------ the B operand
    # B "matrix" [K = Cin*kH*kW][N = oH*oW] of image b is never materialised (conv2d_im2col.nim:62-87 builds it explicitly):
    # element (k, pixel) = input[c][oh*sH + kh - pH][ow*sW + kw - pW], k = (c*kH + kh)*kW + kw.  One wave-instruction gathers one
    # output pixel per lane of ONE k: lane l owns pixels n0 + 2l and n0 + 2l + 1 (two dword loads per piece).  The k part of the
    # address -- (c*H*W + kh*W + kw) * 4 -- is wave-uniform and rides in the load's SGPR offset; the pixel part is a per-lane
    # constant (oh*sH*W + ow*sW) * 4 -- or, where the tap falls into the zero padding (or the pixel lies beyond the image, or k
    # beyond K), the offset 0x80000000 that the bounds check rejects, so the load returns 0 without touching memory.  Which of
    # the two depends on the tap (kh, kw), which is wave-uniform but changes every K-tile: the kH*kW (+1: "nothing") per-lane
    # offset vectors live in LDS and ds_read_addtid_b32 (address = M0 + 4*lane, no VGPR, no VALU op) fetches the right one -- any
    # VALU op in the loop costs ~11 cycles of matrix-pipe time (profiles/r03/asm_probe_v4_fillers.jsonl).  Kernel size, strides and
    # padding are RUN-TIME values (round 6): they only shape the table (built once per tile by a scalar loop over the taps, the
    # four waves taking every fourth tap) and the scalar tap arithmetic; the loop still has no vector instruction.  Wave w owns
    # k = 8w .. 8w+7 of every K-tile: pairs (k, k+2) per lane exactly like the GEMM's pair mode.
    CONV_DELTA = (0, 2, 1, 3, 4, 6, 5, 7)      # piece i = 2*pair + j gathers k = 8w + delta: pairs (0,2) (1,3) (4,6) (5,7)

    def conv_setup(self, again=False):
        """per tile: the geometry, the lanes' pixels, the tap table, srdB, the tap state; again (Cfg.cpers, the switch to the next unit
        inside the K loop): the per-lane LDS write addresses -- the same for every tile -- are left alone"""
        c, p, e, t, st, scr = self.c, self.p, self.p.emit, self.vt, self.s_t, self.s_scr
        B_ = self.ka0.sub(2, 2)
        sH, sW, soW, spH, spW, sCin, sNpix, smagic, sgeo, snt = (scr[i] for i in range(10))
        e("s_load_dwordx8", scr.sub(0, 8), s(0, 2), KA_CONV0)
        e("s_load_dwordx4", scr.sub(8, 4), s(0, 2), KA_CONV1)
        e("s_load_dwordx2", scr.sub(12, 2), s(0, 2), KA_CONV2)
        e("s_waitcnt", lgkmcnt=0)
        # geometry word: kH | kW << 8 | strideH << 16 | strideW << 24; taps word: kH * kW | ceil(1024 / kW) << 16
        e("s_bfe_u32", self.s_kW, sgeo, (8 << 16) | 8)
        e("s_and_b32", self.s_NT, snt, 0xffff)
        e("s_lshr_b32", self.s_M10, snt, 16)
        e("s_bfe_u32", scr[14], sgeo, (8 << 16) | 16)         # strideH
        e("s_lshr_b32", scr[15], sgeo, 24)                    # strideW
        sSH, sSW = scr[14], scr[15]
        lane, tab = t[0], t[1]
        pix = [t[2], t[3]]
        rowb, colb, base = [self.vT[0][0], self.vT[0][1]], [self.vT[0][2], self.vT[0][3]], [self.vT[0][4], self.vT[0][5]]
        e("v_and_b32", lane, 63, v(0))
        e("v_lshlrev_b32", tab, 2, lane)
        e("s_cmp_eq_u32", smagic, 0)
        e("s_cselect_b64", self.s_m, -1, 0)
        for ee in range(2):
            oh, ow = t[4], t[5]
            e("v_lshl_add_u32", pix[ee], lane, 1, self.s_n0)      # this lane's output pixel ee: n0 + 2 * lane + ee
            if ee:
                e("v_add_u32", pix[ee], 1, pix[ee])
            e("v_mul_hi_u32", oh, pix[ee], smagic)                # oh = pix / oW (the pair may straddle two output rows: odd widths)
            e("v_cndmask_b32", oh, oh, pix[ee], self.s_m)         # (oW == 1 travels as magic 0: oh = pix)
            e("v_mul_lo_u32", t[6], oh, soW)
            e("v_sub_u32", ow, pix[ee], t[6])                     # ow = pix % oW
            e("v_mul_lo_u32", t[6], oh, sSH)                      # oh * strideH
            e("v_mul_lo_u32", t[7], ow, sSW)                      # ow * strideW
            e("v_subrev_u32", rowb[ee], spH, t[6])                # input row of tap row 0 (as unsigned: negative = huge)
            e("v_subrev_u32", colb[ee], spW, t[7])
            e("v_mul_lo_u32", t[6], t[6], sW)
            e("v_add_u32", t[6], t[6], t[7])
            e("v_lshlrev_b32", base[ee], 2, t[6])                 # (oh*sH*W + ow*sW) * 4, relative to the window origin of pixel (0, 0)
            e("v_cmp_gt_u32", self.s_pok[ee], sNpix, pix[ee])     # pixels beyond the image (ragged last tile) gather nothing
        e("s_nop", 1)
        # the table: entry r = kh * kW + kw holds, per lane and pixel, the base offset where the tap reads inside the image, the
        # out-of-bounds offset elsewhere.  The same for the 4 waves (they own different k of the same 128 pixels): wave w writes the
        # entries w, w + 4, ...; wave 0 also the "nothing" entry (index taps) that channels beyond Cin select
        L_tap, L_tapd, L_non = p.label("tap"), p.label("tapsdone"), p.label("nonothing")
        sr, skh, skw, soff = st[0], st[2], st[3], st[4]
        e("s_mov_b32", sr, self.s_wave)
        p.place(L_tap)
        e("s_cmp_ge_u32", sr, self.s_NT)
        e("s_cbranch_scc1", L_tapd)
        e("s_mul_i32", skh, sr, self.s_M10)
        e("s_lshr_b32", skh, skh, 10)                             # kh = r / kW
        e("s_mul_i32", skw, skh, self.s_kW)
        e("s_sub_u32", skw, sr, skw)                              # kw = r % kW
        e("s_lshl_b32", soff, sr, 8)
        e("v_add_u32", t[6], soff, tab)
        for ee in range(2):
            e("v_add_u32", t[4], skh, rowb[ee])
            e("v_cmp_gt_u32", VCC, sH, t[4])                      # input row oh*sH + kh - pH exists
            e("v_add_u32", t[5], skw, colb[ee])
            e("v_cmp_gt_u32", self.s_m, sW, t[5])                 # input column exists
            e("s_nop", 1)
            e("s_and_b64", self.s_m, self.s_m, VCC)
            e("s_and_b64", self.s_m, self.s_m, self.s_pok[ee])
            e("s_nop", 0)
            e("v_cndmask_b32", t[7], self.v_oob, base[ee], self.s_m)
            e("ds_write_b32", t[6], t[7], offset=ee * c.TAB_E1)
        e("s_add_u32", sr, sr, 4)
        e("s_branch", L_tap)
        p.place(L_tapd)
        e("s_cmp_lg_u32", self.s_wave, 0)
        e("s_cbranch_scc1", L_non)
        e("s_lshl_b32", soff, self.s_NT, 8)
        e("v_add_u32", t[6], soff, tab)
        e("ds_write_b32", t[6], self.v_oob)
        e("ds_write_b32", t[6], self.v_oob, offset=c.TAB_E1)
        p.place(L_non)
        e("s_waitcnt", lgkmcnt=0)
        e("s_barrier")
        # descriptor: base = B + b * bsB - (pH*W + pW) * 4 (the window origin of output pixel (0, 0), kernel tap (0, 0));
        # every address a valid lane forms lies inside the image -- the bounds field only has to reject v_oob
        img = self.s_img if c.cpers else s(3)
        e("s_mul_hi_u32", st[2], img, scr[10])
        e("s_mul_i32", st[0], img, scr[10])
        e("s_add_u32", st[0], B_[0], st[0])
        e("s_addc_u32", st[2], B_[1], st[2])
        e("s_mul_i32", st[3], spH, sW)
        e("s_add_u32", st[3], st[3], spW)
        e("s_lshl_b32", st[3], st[3], 2)
        e("s_sub_u32", self.srdB[0], st[0], st[3])
        e("s_subb_u32", self.srdB[1], st[2], 0)
        e("s_and_b32", self.srdB[1], self.srdB[1], 0xffff)
        e("s_mov_b32", self.srdB[2], 0x7fffffff)
        e("s_lshl_b32", self.s_W4, sW, 2)
        e("s_mul_i32", self.s_HW4, self.s_W4, sH)
        e("s_mov_b32", self.s_Cin, sCin)
        # LDS write addresses of pair gi, pixel e: x = 2*lane + e, k = 8w + (0, 1, 4, 5)[gi]: L = 2w + (gi & 1), word = (0,0,2,2)[gi]
        e("s_mov_b32", st[0], c.LDS0 + c.ROWP * c.BM)
        for gi in range(0 if again else 4):
            e("s_lshl_b32", st[3], self.s_wave, 1)
            e("s_add_u32", st[3], st[3], gi & 1)
            for ee in range(2):
                xx, rr, ss = t[4], t[5], t[6]
                e("v_lshl_add_u32", xx, lane, 1, ee)
                self.kq_row(rr, xx, t[7])
                self.kq_swz(ss, xx, t[7])
                e("v_xor_b32", ss, st[3], ss)
                e("v_mul_u32_u24", rr, c.ROWP, rr)
                e("v_lshl_add_u32", rr, ss, 4, rr)
                e("v_add_u32", rr, 4 * (0, 0, 2, 2)[gi], rr)
                e("v_add_u32", self.lds_at(self.WB[gi][ee][2])[0], st[0], rr)
                if c.il:
                    continue
                e("v_add_u32", self.WB[gi][ee][0], c.STAGE, self.WB[gi][ee][2])
                e("v_add_u32", self.WB[gi][ee][1], 2 * c.STAGE, self.WB[gi][ee][2])
        # running k of this wave: 8w, + BK per K-tile
        e("s_lshl_b32", self.s_k0, self.s_wave, 3)

    def conv_load_ops(self):
        """per piece: [scalar tap arithmetic] [SGPR offset, table entry -> M0, the two offset vectors from LDS]; then, for every
        piece, [the two gathers]; then the state moves on by BK.  Returns a list of op groups (one per MFMA gap).
        k -> channel c = k / taps (magic multiply: KA_TAB carries floor(2^32 / taps) + 1, 0 for one tap), r = k % taps,
        kh = r / kW = (r * ceil(1024 / kW)) >> 10 (exact for r < 49), kw = r % kW."""
        c, st = self.c, self.s_t
        mgNT = self.ka0[6]
        groups, loads = [], []
        for i in range(8):
            d = self.CONV_DELTA[i]
            g1 = [("ins", "s_add_u32", (st[0], self.s_k0, d), {}),               # k
                  ("ins", "s_mul_hi_u32", (st[1], st[0], mgNT), {}),
                  ("ins", "s_cmp_eq_u32", (mgNT, 0), {}),
                  ("ins", "s_cselect_b32", (st[1], st[0], st[1]), {}),           # c = k / taps
                  ("ins", "s_mul_i32", (st[2], st[1], self.s_NT), {}),
                  ("ins", "s_sub_u32", (st[0], st[0], st[2]), {}),               # r = k % taps
                  ("ins", "s_mul_i32", (st[2], st[0], self.s_M10), {}),
                  ("ins", "s_lshr_b32", (st[2], st[2], 10), {}),                 # kh = r / kW
                  ("ins", "s_mul_i32", (st[3], st[2], self.s_kW), {}),
                  ("ins", "s_sub_u32", (st[5], st[0], st[3]), {})]               # kw = r % kW
            g2 = [("ins", "s_mul_i32", (st[3], st[1], self.s_HW4), {}),
                  ("ins", "s_mul_i32", (st[4], st[2], self.s_W4), {}),
                  ("ins", "s_add_u32", (st[3], st[3], st[4]), {}),
                  ("ins", "s_lshl_b32", (st[4], st[5], 2), {}),
                  ("ins", "s_add_u32", (self.s_koff[i], st[3], st[4]), {}),  # (c*H*W + kh*W + kw) * 4
                  ("ins", "s_cmp_lt_u32", (st[1], self.s_Cin), {}),
                  ("ins", "s_cselect_b32", (st[0], st[0], self.s_NT), {}),   # channels beyond Cin (k >= K): the "nothing" entry
                  ("ins", "s_lshl_b32", (M0, st[0], 8), {}),
                  ("ins", "s_nop", (0,), {}),                                # (S_MOV to M0 -> LDS add-TID instruction: 1 wait state)
                  ("ldsr", "ds_read_addtid_b32", (self.vB0[i],), {}, ("T", i)),
                  ("ldsr", "ds_read_addtid_b32", (self.vB1[i],), {"offset": c.TAB_E1}, ("T", i))]
            groups += [g1, g2]
            loads.append([("lgwait", {("T", i)}), ("loadBc", i, 0), ("loadBc", i, 1)])
        groups += loads
        groups.append([("ins", "s_add_u32", (self.s_k0, self.s_k0, c.BK), {})])
        return groups

    def conv_store_ops(self, k):
        """tile data in the B staging registers -> LDS stage index k; returns op groups"""
        out = []
        for gi in range(4):
            P, Q = self.stB[2 * gi], self.stB[2 * gi + 1]
            for ee in range(2):
                g = [("vmwait", ("B", 2 * gi + 1, 1))] if ee == 0 else []
                g.append(self.w2(self.WB[gi][ee][k], P[ee], Q[ee]))
                out.append(g)
        return out

    def run_op(self, o):
        if o[0] != "loadBc":
            return super().run_op(o)
        if "loads" not in self.c.ablate:
            self.p.emit("buffer_load_dword", self.stB[o[1]][o[2]], (self.vB0, self.vB1)[o[2]][o[1]], self.srdB, self.s_koff[o[1]], offen=True)
            self.vm_issue(("B", o[1], o[2]))

    def staging_units(self, wr_k):
        """B first (its gathers were requested a tile ago and are needed soonest): stores, then the scalar tap state and the offset
        vectors of tile t+2, its 16 gathers, then A's pieces; one unit per gap"""
        a_units = []
        for pi in range(self.c.NPA):
            a = self.store_A_piece(pi, ops=[], k=wr_k)
            a_units += [a[:2], [a[2]], [("loadA", pi)]]
        return self.conv_store_ops(wr_k) + self.conv_load_ops() + a_units

    # ------------------------------------------------------------------ unit walkers (Cfg.cpers)
    def next_unit(self, L_none):
        """Cfg.cpers: the workgroup's next unit -> s_img, s_m0, s_n0 (L_none when there is none).  KA_SCHED2 carries, for these kernels,
        +4 the tiles of one image, +8 their magic number, +12 the stride (= workgroups), +16 the units of the launch (images x tiles).
        Clobbers s_scr[0..7] (dead outside a tile body's load section) and s_t[0..5]."""
        e, st, sc = self.p.emit, self.s_t, self.s_sc
        e("s_load_dwordx8", sc, s(0, 2), KA_SCHED2)
        e("s_waitcnt", lgkmcnt=0)
        e("s_cmp_ge_u32", self.s_tcur, sc[4])
        e("s_cbranch_scc1", L_none)
        self.udiv(self.s_img, self.s_tcur, sc[2])
        e("s_mul_i32", st[4], self.s_img, sc[1])
        e("s_sub_u32", st[4], self.s_tcur, st[4])                     # the tile inside the image
        e("s_add_u32", self.s_tcur, self.s_tcur, sc[3])
        e("s_load_dwordx8", sc, s(0, 2), KA_SCHED)
        e("s_waitcnt", lgkmcnt=0)
        self.tile_origin(st[4])

    def switch_tile(self, L_out):
        """pipe_switch: on to the workgroup's next unit, or to L_out when there is none.  Every wave that gets here has passed the barrier of the tile body it
        comes from, and a wave only reaches that barrier after its last look at the tap table (the table reads of a body precede its
        gathers, the gathers the barrier): the table of the tile being finished can be overwritten at once; conv_setup's own barrier
        stands between the new table's writes and its first reads.  Scalar tap state, srdB and srdC move to the next unit; the C
        addresses of the tile being finished were put aside first."""
        e, st = self.p.emit, self.s_t
        e("s_load_dword", st[0], s(0, 2), KA_SCHED2 + 16)
        e("s_waitcnt", lgkmcnt=0)
        e("s_cmp_lt_u32", self.s_tcur, st[0])
        e("s_cbranch_scc0", L_out)
        self.pipe_c_addr()
        self.next_unit(L_out)
        self.a_descriptor()
        self.b_descriptor(again=True)
        self.c_descriptor()
