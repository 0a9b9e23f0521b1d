// The launch plan of a conv: which kernel form, tile, statistics slots, flat tile list and input staging a launch gets.  Decided
// here once, on the host, from the layer's shape and options, the precision mode, the batch, the column count and the CU count;
// conv_call (conv_call.hip) fills its input and builds the kernel arguments to match; Model::conv and the test hooks size their
// buffers from the plan and hand it to launch_conv (conv_f16x3.hip), whose launchers carry it out.  No HIP calls: the plan is a pure function of its inputs (tests/test_conv_plan_cpu.py runs it without a GPU).
//
// What decides an utterance's bits must not depend on the batch or the lengths: the MFMA family of a layer (the 16x16x32 forms
// by shape alone), whether its input goes through a pre-split image (by shape alone) and the width of its statistics slots
// (128 columns for every 32x32x16 form, 64 for the 16x16x32 ones).  The rest -- tile width, wave layout, the narrow forms, the
// flat tile list -- may follow the grid: those forms are bit-identical to each other (tests/test_gpu_kernels.py).
#include "kx_common.h"

namespace kx {

// the direct-A conv (conv_f16x3_da.hip): 128-row weight tiles, stride 1, a window of at most 384 columns, not the merged columns
static bool da_eligible(int BM, int K, int dil, int stride, bool merged) {
    return BM == 128 && stride == 1 && !merged && (K - 1) * dil + 256 <= 384;
}

// tap counts of the f16f8 forms of the 16x16x32 loop (conv_f16x3_da_f8.hip)
static bool f8_taps(int K, int dil) { return (K == 11 || K == 7 || K == 3) && (K - 1) * dil <= 64; }

// Shapes of the 16x16x32 forms (conv_f16x3_da_s16.hip, _f8.hip): snake resblock convs with an even number of 16-channel chunks;
// 11 taps always, the un-dilated 7-tap ones (measured: the big 7-tap launches gain 3 % on this form, the dilated ones lose 3 %:
// profiles/r03_s16_form.txt).  pmode: 0 = f16x3, 1 = reduced precision (never this form), 2 = f16f8 (the layer carries an
// 8-bit cross image: every 7-tap conv takes the form -- with two MFMA-equivalents per product the dilated ones gain 18 % on it
// -- and the 3-tap ones too: bound by their transform, they still gain 6 % from the hardware cosine and the shorter MFMA stream).
static bool s16_shape(int BM, int K, int dil, int stride, int act, int n_chunks16, bool merged, int pmode) {
    const bool taps = K == 11 || (K == 7 && dil == 1) || (pmode == 2 && f8_taps(K, dil));
    return BM == 128 && stride == 1 && !merged && pmode != 1 && act == ACT_SNAKE && taps && (K - 1) * dil <= 64 && n_chunks16 >= 2 &&
           (n_chunks16 & 1) == 0;
}

bool conv16_f8_layer(int BM, int rows, int K, int n_chunks16) {
    // (the activation is a property of the call, not of the weights: a few leaky 3-tap convs of the predictor get an image they
    // never use; the 3-tap convs of more than 256 rows are not the generator's snake resblocks)
    return BM == 128 && f8_taps(K, 1) && (K != 3 || rows <= 256) && n_chunks16 >= 2 && (n_chunks16 & 1) == 0;
}

ConvPlan conv_plan(const ConvLaunch& c) {
    ConvPlan p{};
    p.bm = c.BM;
    p.act = c.act;
    p.vt = 1;
    p.cols = c.cols;
    // InstanceNorm partial sums ride in the epilogue of plain, non-accumulating stores
    const bool stats = c.stats && c.store == ST_NORMAL && !c.accum;
    // slots of stat_cols columns; stat_tiles of them per row, over tiles of p.bn columns
    auto set_stats = [&](int stat_cols) {
        if (!stats) return;
        p.stat_cols = stat_cols;
        p.stat_tiles = (p.cols + p.bn - 1) / p.bn * (p.bn / stat_cols);
    };
    if (c.mode == CONV_F32) {  // conv1d_mfma_kernel: 128 x 128 (2 x 2 waves) or BM x 256 (1 x 4)
        p.form = FORM_F32;
        p.bn = c.BM == 128 ? 128 : 256;
        set_stats(64);
        return p;
    }
    const int route = c.force & 3;  // test overrides: FORCE_LDS, FORCE_DA
    const int pmode = c.prec1 ? 1 : (c.f8 ? 2 : 0);

    // Layers whose input window many row tiles stage get a pre-split image of the input (conv_f16x3_pre.hip): >= 4 row tiles per
    // window.  At batch 64 the 512-row layers (the predictor's F0 / N convs, decode.3) gain from it what their six extra passes
    // cost (profiles/r05_experiments_not_kept.txt: 113.32 vs 113.28 ms); at batch 1 they then take the narrow form (64 workgroups
    // instead of 16 on the forward's critical path), which is what the row count is set by.
    const bool pre_form = c.stride == 1 && c.K >= 2 && !c.in_up2 && c.act != ACT_SNAKE && !c.prec1 &&
                          da_eligible(c.BM, c.K, c.dil, c.stride, false);
    p.pre = (c.mode == CONV_F16X3 || c.mode == CONV_F16F8) && c.image && pre_form && (c.image == 2 || c.rows >= 512);

    // k = 1 GEMMs over a short axis (the token axis): the columns of all B utterances form one merged space
    p.merged = c.B > 1 && c.K == 1 && c.stride == 1 && c.pad == 0 && !c.in_up2 && !c.norm && c.store != ST_UPSCATTER && !c.stats &&
               c.merge_T > 0 && c.merge_T <= 512;
    if (p.merged) p.cols = c.B * c.merge_T;

    if (c.BM != 128) {  // 64- and 32-row weight tiles: the LDS-DMA form, 1 x 4 waves
        p.form = FORM_LDS;
        p.bn = 256;
        p.wm = 1;
        p.wn = 4;
        p.pf = c.stride == 1 && (c.K - 1) * c.dil <= 128;  // (the prefetching build: a window of at most BN + 128 columns)
        set_stats(64);
        return p;
    }

    // k = 1 GEMMs (ALBERT, projections, LSTM input products)
    if (c.K == 1 && c.stride == 1 && !stats && !c.in_up2 && c.n_chunks16 >= 3 && c.act != ACT_SNAKE) {
        const long tiles = (long)((p.cols + 127) / 128) * ((c.rows + 127) / 128);  // 128 x 128 tiles of one utterance (merged: all)
        if (route != FORCE_LDS && !c.norm && c.store != ST_UPSCATTER) {
            // the direct-A GEMM (conv_f16x3_dag.hip).  At most half as many 128 x 128 tiles as CUs: the narrow form, 128 x 32
            // (measured by batch, 128 x 128 / narrow: 1: 11.85 / 10.55 ms, 4: 16.74 / 15.73, 16: 36.6 / 36.5; at 32 and 64 no
            // launch qualifies: on the big grids it costs four times the weight traffic), whose offsets into the input are 32 bits
            const long wgs = tiles * (p.merged ? 1 : c.B);
            const bool narrow_ok = (c.x_bs * c.B + 16L * c.x_ld) * 4 < (1L << 31);  // (one 16-channel chunk past the last utterance)
            p.form = narrow_ok && 2 * wgs <= c.cus ? FORM_DAGN : FORM_DAG;
            p.bn = p.form == FORM_DAGN ? 32 : 128;
            return p;
        }
        // the virtual-tap LDS-DMA form: two 16-channel chunks per super-chunk on large grids (48 KiB of LDS, three workgroups per
        // CU), three on small ones (fewer barriers per unit of work; every workgroup is resident anyway)
        p.form = FORM_LDS;
        p.bn = 128;
        p.wm = 2;
        p.wn = 2;
        p.pf = 1;
        p.vt = tiles > 2L * c.cus ? 2 : 3;
        return p;
    }

    // Tile: 256 columns by default; 128 for short sequences (LDS-DMA 2 x 2 waves); and for small grids (batch 1: 256-column tiles
    // would not even give every CU one workgroup) 128 with each wave spanning 128 columns, so that the fused statistics cover
    // the same 128-column groups in the same order as on the 256-column tile (batch invariance).  Fused statistics keep their
    // 128-column slots whatever the grid, so the short-sequence tile (64-column slots) is not taken for them.
    const bool da = route != FORCE_LDS && da_eligible(c.BM, c.K, c.dil, c.stride, p.merged);
    const bool small = (long)((p.cols + 255) / 256) * ((c.rows + 127) / 128) * c.B < 256;
    if (route != FORCE_LDS && !(c.force & FORCE_NO_S16) && s16_shape(c.BM, c.K, c.dil, c.stride, c.act, c.n_chunks16, p.merged, pmode)) {
        // the 16x16x32 forms (f16f8: their F8 forms): 192 columns on chip-filling grids, 128 on small ones; 64-column slots
        p.form = pmode == 2 ? FORM_DA_F8 : FORM_DA_S16;
        p.kt = c.K;
        p.bn = small && route != FORCE_DA ? 128 : 192;
        set_stats(64);
    } else if (!da || (route != FORCE_DA && c.cols <= 160 && !stats)) {
        // the LDS-DMA form: 128 x 128 with 2 x 2 waves on short sequences, 4 x 1 (one wave per 128 columns) on small grids
        p.form = FORM_LDS;
        const bool short_seq = c.cols <= 160 && !stats;
        p.bn = !short_seq && !small ? 256 : 128;
        p.wm = !short_seq && small ? 4 : 2;
        p.wn = !short_seq && small ? 1 : 2;
        p.pf = c.stride == 1 && (c.K - 1) * c.dil <= 128;
        set_stats(p.bn / p.wn);
    } else {
        // the direct-A conv, 256 columns (128 on small grids), 128-column slots
        p.bn = small && route != FORCE_DA ? 128 : 256;
        set_stats(128);
        const bool w64 = (c.K - 1) * c.dil <= 64;  // (the unrolled forms stage a window of BN + 64 columns)
        if (p.pre) {
            // small grids: the narrow form without staging, 32 rows x 128 columns per workgroup; else the pre-split image staged
            // into the 128 x bn tile (the activation is in the image), unrolled for 3 taps
            const bool narrow = p.bn == 128 && !c.prec1 && c.rows % 32 == 0 && c.K <= 12 && c.epi == EPI_NONE &&
                                (c.store == ST_NORMAL || c.store == ST_UPSCATTER) && (long)c.n_chunks16 * c.K < 5000;
            p.form = narrow ? FORM_DAPN : FORM_DA_PRE;
            p.act = ACT_NONE;
            p.kt = c.K == 3 && w64 ? 3 : 0;
        } else {
            // compile-time tap counts for the resblock convs (the transform dealt out between the MFMAs), run-time ones for the
            // rest; the 256-column tile's unrolled forms run with the waves as 2 x 2 (bit-identical to 4 x 1; not built for the
            // reduced-precision forms, which are bound by the transform)
            const bool unrolled = w64 && ((c.act == ACT_SNAKE && (c.K == 11 || c.K == 7 || c.K == 3)) || (c.act == ACT_LEAKY && c.K == 3));
            p.kt = unrolled ? c.K : 0;
            p.p1 = c.prec1 != 0;
            p.bf = c.prec1 == 2;
            p.form = unrolled && p.bn == 256 && !c.prec1 && !(c.force & FORCE_DA_4X1) ? FORM_DA_W2 : FORM_DA;
        }
    }
    // ragged batches: the direct-A forms take a flat list of the live tiles instead of a (longest length) x B grid
    const bool flat_form = p.form != FORM_LDS;
    p.flat_bn = flat_form && c.B > 1 && p.cols > 0 ? p.bn : 0;
    return p;
}

}  // namespace kx
