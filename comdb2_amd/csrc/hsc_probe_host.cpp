// hsc_probe_host.cpp -- the probe dispatch: a hsc_probe_batch on a built
// window becomes the kernel launches of one of the probe paths, on the
// context's stream, in the scratch of the stream's lane.  Reaches the context
// only through hsc_ctx.h and the kernels only through the launch_* wrappers of
// hsc_internal.h.  Host code only, compiled as plain C++ like
// hsc_graph_host.cpp.
//
// Timing (hsc_enable_timing): six events ev[0..5] bound five legs, reported as
// locate | plan | scatter | join | pack (collect_timing).  What each path
// launches in which leg ("-": an empty leg, its two events back to back):
//
//   path                           locate          plan  scatter  join     pack
//   direct (probe_narrow)          verdict clear   -     -        probe    pack
//                                                                 + delta
//   narrow tiles, column           locate          -     -        join     delta (+ pack
//                                                                          if it ran)
//   narrow tiles, plan             locate          plan  -        join     delta (+ pack)
//   narrow / compact tiles with    locate          -     -        -        delta into flags
//   nothing to join                                                        + pack_flags
//   compact tiles                  bound mapping   plan  -        join     delta (+ pack)
//                                  + locate
//   wide pipeline (probe_tiles)    bound mapping,  plan  scatter  join     delta + pack
//                                  clears, locate
//
// The wide pipeline's bound mapping is compact_probes on a compact window and
// narrow_codes on a narrow one (HSC_LAYOUT_NARROW_CODES, or tile rows that do
// not fit 8 bytes); a wide window has none.
#include "hsc_ctx.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

// The batch's six timing events.  One per batch (probe_lane); mark(k) records
// every event up to k that the batch has not recorded yet on the stream, so a
// path names only the ends of the legs it fills.  With timing off it tests one
// bool.
struct PhaseMarker {
    hsc_ctx *c;
    const bool on;
    int next = 0;
    explicit PhaseMarker(hsc_ctx *c) : c(c), on(c->timing) {}
    int mark(int k)
    {
        if (!on) return HSC_OK;
        for (; next <= k; ++next) {
            if (!c->ev[next]) HIPCHK(c, hipEventCreate(&c->ev[next]));
            HIPCHK(c, hipEventRecord(c->ev[next], c->stream));
        }
        return HSC_OK;
    }
};

WinView win_view(hsc_ctx *c)
{
    WinView w{};
    w.words = c->d_words.as<uint64_t>();
    w.stride = c->cap;
    w.lsn = c->d_lsn.as<uint64_t>();
    w.gid = c->d_gid.as<uint32_t>();
    w.gstart = c->d_gstart.as<uint32_t>();
    w.gend = c->d_gend.as<uint32_t>();
    w.tmax = c->d_tmax.as<uint64_t>();
    w.table_max = c->d_table_max.as<uint64_t>();
    w.sp_g = c->d_sp_g.as<uint32_t>();
    w.sp_w = c->d_sp_w.as<uint64_t>();
    w.n = (uint32_t)c->n;
    w.ntiles = c->ntiles;
    w.ntables = (uint32_t)c->table_names.size();
    w.W = c->W;
    w.log2T = c->log2T;
    w.levels = c->levels;
    w.gbits = 0;
    while (w.gbits < 32 && ((size_t)1 << w.gbits) < c->groups.size()) w.gbits++;
    return w;
}

// A tile view of the window (c->wn, c->wc) with the table maxima of w, which
// change with every append.  gbits stays the view's own 0: only the wide
// pipeline's locate reads it (key_prefix in k_locate), and only its compact
// caller has group ids to prefix (probe_ccodes sets it).
WinView with_tables(WinView view, const WinView &w)
{
    view.table_max = w.table_max;
    view.ntables = w.ntables;
    return view;
}

// Range probes of the batch against the delta run (appends since the last
// build) into the path's verdict target, before its pack.
int probe_delta(hsc_ctx *c, uint8_t *target)
{
    if (!c->raw_probe.n) return HSC_OK;
    if (c->fn) HIPCHK(c, launch_probe_delta(frozen_view(c), c->raw_probe, target, c->stream));
    if (c->dn) HIPCHK(c, launch_probe_delta(delta_view(c), c->raw_probe, target, c->stream));
    return HSC_OK;
}

// the batch's delta probe will mark verdict bytes (then a pack pass builds the bitmap)
bool pack_after_delta(const hsc_ctx *c) { return c->raw_probe.n && (c->fn || c->dn); }

// The end of a bucketed path whose join marked the verdict bytes (and, with
// no delta run, the bitmap): the delta probe marks bytes only, so a pack pass
// follows if it ran (delta = pack_after_delta(c), which the caller's
// work.bitmap went by).
int tail_verdict(hsc_ctx *c, PhaseMarker &t, const hsc_probe_batch *b, bool delta)
{
    HIPCHK_RC(c, t.mark(4));
    HIPCHK_RC(c, probe_delta(c, b->verdict));
    if (delta) HIPCHK(c, launch_pack(b->verdict, (uint32_t)b->n_txn, b->bitmap, c->stream));
    return t.mark(5);
}

// The end of a bucketed path with nothing to join: the delta probe marks the
// locate's flags, pack_flags moves them into the verdict bytes and the bitmap.
int tail_flags(hsc_ctx *c, PhaseMarker &t, const hsc_probe_batch *b, uint8_t *flags)
{
    HIPCHK_RC(c, t.mark(4));
    HIPCHK_RC(c, probe_delta(c, flags));
    HIPCHK(c, launch_pack_flags(flags, (uint32_t)b->n_txn, b->verdict, b->bitmap, c->stream));
    return t.mark(5);
}

// Narrow layout: one kernel answers every range and table lock.
int probe_narrow(hsc_ctx *c, const hsc_probe_batch *b, const WinView &w, const ProbeView &p,
                 PhaseMarker &t)
{
    hipStream_t s = c->stream;
    c->probe_ntiles = 0;
    NarrowView nv = c->nv;
    nv.table_max = w.table_max;
    nv.ntables = w.ntables;
    HIPCHK_RC(c, t.mark(0));
    if (b->n_txn) HIPCHK(c, hipMemsetAsync(b->verdict, 0, b->n_txn, s));
    HIPCHK_RC(c, t.mark(3));
    HIPCHK(c, launch_probe_narrow(nv, p, b->verdict, s));
    HIPCHK_RC(c, probe_delta(c, b->verdict));
    HIPCHK_RC(c, t.mark(4));
    HIPCHK(c, launch_pack(b->verdict, (uint32_t)b->n_txn, b->bitmap, s));
    return t.mark(5);
}

#ifdef HSC_STAMPS
// Diagnostic builds: phase durations of the locate (np0 stamps) and the join
// (np1 stamps), median over blocks, in shader cycles; clears the stamps.
int stamp_report(hsc_ctx *c, const ProbeWork &work, uint32_t max_items, int np0, int np1)
{
    hipStream_t s = c->stream;
    if (!work.stamps) return HSC_OK;
    std::vector<uint64_t> h(2 * 8192 * 8);
    HIPCHK(c, hipMemcpyAsync(h.data(), work.stamps, 8 * h.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const uint32_t nb[2] = {8 * ((work.G + 7) / 8), max_items};
    const int np[2] = {np0, np1};
    for (int k = 0; k < 2; ++k) {
        fprintf(stderr, "[stamps] %s blocks %u:", k ? "join" : "locate", nb[k]);
        uint64_t t0 = ~0ull, t1 = 0;
        for (uint32_t b = 0; b < nb[k] && b < 8192; ++b) {
            const uint64_t *r = &h[((size_t)k * 8192 + b) * 8];
            if (!r[0]) continue;
            t0 = std::min(t0, r[0]);
            t1 = std::max(t1, r[np[k] - 1]);
        }
        for (int q = 1; q < np[k]; ++q) {
            std::vector<uint64_t> d;
            for (uint32_t b = 0; b < nb[k] && b < 8192; ++b) {
                const uint64_t *r = &h[((size_t)k * 8192 + b) * 8];
                if (r[q] && r[q - 1]) d.push_back(r[q] - r[q - 1]);
            }
            std::sort(d.begin(), d.end());
            fprintf(stderr, " p%d %llu", q, d.empty() ? 0ull : (unsigned long long)d[d.size() / 2]);
        }
        std::vector<uint64_t> st;
        for (uint32_t b = 0; b < nb[k] && b < 8192; ++b) {
            const uint64_t *r = &h[((size_t)k * 8192 + b) * 8];
            if (r[0]) st.push_back(r[0] - t0);
        }
        std::sort(st.begin(), st.end());
        fprintf(stderr, " | span %llu, start p50 %llu p90 %llu\n", (unsigned long long)(t1 - t0),
                st.empty() ? 0ull : (unsigned long long)st[st.size() / 2],
                st.empty() ? 0ull : (unsigned long long)st[st.size() * 9 / 10]);
    }
    HIPCHK(c, hipMemsetAsync(work.stamps, 0, 8 * h.size(), s));
    return HSC_OK;
}
#endif

// Scratch of the two bucketed pipelines (narrow tiles, compact tiles) for a
// batch in chunks of work.chunk probes: sizes the buffers, points work at them
// and sets work.G.  rec_bytes: a chunk-sorted record (16 narrow, 64 compact);
// cm_bytes: an entry of the chunk-major rows (8 narrow, 4 compact).
// -> max_items (the join's items at most), flags (the batch's conflict flags).
int bucket_scratch(hsc_ctx *c, const hsc_probe_batch *b, const ProbeView &p, uint32_t ntiles,
                   size_t rec_bytes, size_t cm_bytes, ProbeWork &work, uint32_t &max_items,
                   uint8_t *&flags)
{
    const uint32_t nt = std::max<uint32_t>(ntiles, 1);
    work.lds_mode = 1;
    work.G = (uint32_t)std::max<size_t>(1, (std::max<size_t>(p.n, p.n_lock) + work.chunk - 1) / work.chunk);
    const size_t n1 = std::max<uint32_t>(p.n, 1);
    HIPCHK(c, c->w_hist.ensure(4 * (size_t)hist_stride(work.G) * nt));
    // tile buckets of kTileCap records, then the overflow area (at most 2n
    // records spill); join items: one per tile + the overflow chunks (each hot
    // tile rounds its own run up: at most 2 ceil(2n / kJoinChunk) of them)
    HIPCHK(c, c->w_counts.ensure(4 * ((size_t)nt + 1)));
    HIPCHK(c, c->w_bucket.ensure(4 * ((size_t)nt + 1)));
    HIPCHK(c, c->w_items.ensure(4 * std::max<size_t>((size_t)nt + 1, 4)));
    const uint32_t extra_items = 2 * (uint32_t)((2 * n1 + kJoinChunk - 1) / kJoinChunk);
    max_items = nt + extra_items;
    HIPCHK(c, c->w_item_desc.ensure(16 * (size_t)extra_items + 16));
    // chunk-sorted records: each chunk's records in an area of its own, tile
    // runs found by the join through the plan's scan (no scatter pass)
    HIPCHK(c, c->w_tcode2.ensure(2 * (size_t)hist_stride(work.G) * nt));  // cst: run starts
    HIPCHK(c, c->w_tcode.ensure(cm_bytes * (size_t)work.G * ((nt + 3) & ~3u)));  // chunk-major rows
    HIPCHK(c, c->w_trecs.ensure(rec_bytes * 2 * (size_t)work.chunk * work.G));
    work.cst = c->w_tcode2.as<uint16_t>();
    work.hist = c->w_hist.as<uint32_t>();
    work.counts = c->w_counts.as<uint32_t>();
    work.bucket_off = c->w_bucket.as<uint32_t>();
    work.item_off = c->w_items.as<uint32_t>();
    work.item_desc = c->w_item_desc.as<uint4>();
#ifdef HSC_STAMPS
    static DBuf stamp_buf;
    if (getenv("HSC_STAMPS")) {
        if (!stamp_buf.p) {
            HIPCHK(c, stamp_buf.ensure(8 * 2 * 8192 * 8));
            HIPCHK(c, hipMemsetAsync(stamp_buf.p, 0, 8 * 2 * 8192 * 8, c->stream));
        }
        work.stamps = stamp_buf.as<uint64_t>();
    }
#endif
    // conflict flags: internal, all zero between batches (the pack clears them)
    const size_t had = c->w_vflags.bytes;
    HIPCHK(c, c->w_vflags.ensure((std::max<size_t>(b->n_txn, 1) + 15) & ~(size_t)15));
    if (c->w_vflags.bytes != had) HIPCHK(c, hipMemsetAsync(c->w_vflags.p, 0, c->w_vflags.bytes, c->stream));
    flags = c->w_vflags.as<uint8_t>();
    return HSC_OK;
}

// Narrow tiles (dense batch): locate (codes, snapshot ranks, per-chunk tile
// histograms) -> column scan + plan -> scatter (16-byte records) -> join
// (8-byte rows) -> pack.
int probe_ntiles(hsc_ctx *c, const hsc_probe_batch *b, const WinView &wn, const ProbeView &p,
                 PhaseMarker &t)
{
    hipStream_t s = c->stream;
    c->probe_ntiles = wn.ntiles;
    c->probe_buckets = true;
    ProbeWork work{};
    if (!c->d_fulljoins.p) {
        HIPCHK(c, c->d_fulljoins.ensure(8));
        HIPCHK(c, hipMemset(c->d_fulljoins.p, 0, 8));
    }
    work.full_joins = c->d_fulljoins.as<uint32_t>();
    work.wave_fallbacks = work.full_joins + 1;
    // chunks of narrow_tiles_chunk() probes (at most kMaxChunks: the caller
    // sends larger batches down the code-tile path); 16-byte records,
    // chunk-major rows of {kept records' run and count, located records}
    work.chunk = narrow_tiles_chunk();
    uint32_t max_items;
    uint8_t *flags;
    HIPCHK_RC(c, bucket_scratch(c, b, p, wn.ntiles, 16, 8, work, max_items, flags));
    work.cursor = c->w_cursor.as<uint32_t>();
    work.item_tile = c->w_item_tile.as<uint32_t>();
    NarrowTiles ntl{};
    ntl.key32 = c->d_key32.as<uint32_t>();
    ntl.rank32 = c->d_rank32.as<uint32_t>();
    ntl.rank_lsn32 = c->rank_lsn32;
    ntl.rank_base = c->rank_base;
    ntl.cdir = c->cdir;
    ntl.tdir = c->tdir;
    ntl.trad = c->trad_m ? c->d_trad.as<uint32_t>() : nullptr;
    ntl.trad_m = c->trad_m;
    ntl.trad16 = c->trad_m ? c->d_trad16.as<uint16_t>() : nullptr;
    ntl.trad_shift = c->trad_shift;
    ntl.recs = c->w_trecs.as<uint4>();
    narrow_recent_view(ntl, c->d_recent.as<uint32_t>(), wn.ntiles, c->slot_qshift);
    // The batch's path.  Balanced window: no plan -- the locate clears the
    // verdict bytes, the join scans its tiles' columns, runs a tile of more
    // than kTileCap records in rounds inside its one block and moves the
    // flags.  The plan and its overflow blocks stay for a skewed window (the
    // bucket table in log mode) and while a batch of the last kHotBatches had
    // such a tile: the kernels of either path store the batch's number into
    // the hot word, which is read here as it stands (a late store only delays
    // the switch; both paths give the same verdicts).
    const bool joins = p.n && wn.ntiles;
    const bool delta = pack_after_delta(c);
    bool column = false;
    if (joins) {
        if (!c->h_hot.p) {  // two words: hot, wide (hsc_ctx.h)
            if (c->h_hot.ensure(16, true, true)) return ctx_fail(c, HSC_ENOMEM, "hot word");
            c->h_hot.as<volatile uint64_t>()[0] = 0;
            c->h_hot.as<volatile uint64_t>()[1] = 0;
        }
        work.hot = (uint64_t *)c->h_hot.dp;
        work.wide = work.hot + 1;
        work.batch = ++c->nt_batch;
        const uint64_t hot = *c->h_hot.as<volatile uint64_t>();
        column = !c->trad_log && !(hot && work.batch - hot <= hsc_ctx::kHotBatches);
        (column ? c->nt_column : c->nt_plan)++;
    }
    if (column) {
        work.vout = b->verdict;
        work.n_txn = (uint32_t)b->n_txn;
        work.bitmap = delta ? nullptr : b->bitmap;
    }
    HIPCHK_RC(c, t.mark(0));
    // the table's layout goes with the locate instance: two-word entries
    // where its filter makes located != kept, one word otherwise
    if (narrow_locate_fast(c->nv, ntl, p))
        work.cmx = c->w_tcode.as<uint2>();
    else
        work.cm = c->w_tcode.as<uint32_t>();
    int shape = -1;
    HIPCHK(c, launch_locate_t(c->nv, wn, p, work, ntl, flags, s, &shape));
    if (shape >= 0) (shape ? c->nt_fast : c->nt_general)++;
    HIPCHK_RC(c, t.mark(1));
    if (column) {
        HIPCHK_RC(c, t.mark(3));  // (no plan, no scatter)
        // a wave per tile for what a fast locate's filter left, unless a batch
        // of the last kHotBatches was wide (the word as it stands: a late
        // store only delays the switch, both joins give the same verdicts)
        const uint64_t wide = c->h_hot.as<volatile uint64_t>()[1];
        const bool wave = work.cmx && !(wide && work.batch - wide <= hsc_ctx::kHotBatches);
        (wave ? c->nt_wave : c->nt_block)++;
        if (wave)
            HIPCHK(c, launch_join_wave(work, ntl, wn.n, wn.ntiles, flags, s));
        else
            HIPCHK(c, launch_join_col(work, ntl, wn.n, wn.ntiles, flags, s));
        HIPCHK_RC(c, tail_verdict(c, t, b, delta));
    } else if (joins) {
        // the plan writes the verdict bytes (and bitmap words) from the
        // locate's flags; the join and the delta probe then mark the verdict
        // itself, the join its bitmap bits too (no pack pass unless the delta
        // probe ran: it marks bytes only)
        work.bitmap = delta ? nullptr : b->bitmap;
        HIPCHK(c, launch_plan_s(work, wn.ntiles, c->w_items.as<uint32_t>(), s, flags,
                                (uint32_t)b->n_txn, b->verdict));
        HIPCHK_RC(c, t.mark(3));  // (no scatter)
        // blocks past the tiles for the hot tiles' overflow items: 512, or 2048
        // on a skewed window (the bucket table took log mode: Zipf keys crowd
        // a few tiles -- r03: config 5 one stream 83 -> 80 us with 2048, while
        // config 2's idle extra blocks cost its overlapped batch)
        const uint32_t extra = c->trad_log ? 2048u : 512u;
        HIPCHK(c, launch_join_t(work, ntl, wn.n, wn.ntiles, max_items, b->verdict, s, extra));
        HIPCHK_RC(c, tail_verdict(c, t, b, delta));
    } else {
        HIPCHK_RC(c, tail_flags(c, t, b, flags));
    }
#ifdef HSC_STAMPS
    HIPCHK_RC(c, stamp_report(c, work, max_items, 6, 4));
#endif
    return HSC_OK;
}

// Compact tiles (dense or sparse batch over a compact window): code bounds
// (compact_probes) -> locate (gid || code keys, end tiles, 64-byte probe
// entries) -> plan -> scatter (4-byte bucket entries) -> join -> pack.
int probe_ctiles(hsc_ctx *c, const hsc_probe_batch *b, const WinView &w, const ProbeView &p,
                 PhaseMarker &t)
{
    hipStream_t s = c->stream;
    CTiles ct = c->ctv;
    c->probe_ntiles = ct.ntiles;
    c->probe_buckets = true;
    ProbeWork work{};
    const size_t n1 = std::max<uint32_t>(p.n, 1);
    HIPCHK(c, c->p_code_lo.ensure(8 * (size_t)c->ct.WC * n1));
    HIPCHK(c, c->p_code_hi.ensure(8 * (size_t)c->ct.WC * n1));
    // chunk-sorted 64-byte records (the read set number shares its word with
    // the record kind: the caller sends batches of >= 2^30 read sets down the
    // wide pipeline), one-word chunk-major entries
    work.chunk = ctiles_chunk();
    uint32_t max_items;
    uint8_t *flags;
    HIPCHK_RC(c, bucket_scratch(c, b, p, ct.ntiles, 64, 4, work, max_items, flags));
    work.cm = c->w_tcode.as<uint32_t>();
    ct.recs = c->w_trecs.as<uint32_t>();
    ct.np = p.n;
    const WinView wt = with_tables(c->wc, w);  // tile maxima of the same 2048-row tiles
    HIPCHK_RC(c, t.mark(0));
    // (measured: the bound mapping fused into the locate -- code bounds kept in
    // registers -- ran 83 us against 67 us for the two kernels on config 3)
    PointHash ph{};
    if (c->cph_nb) {
        ph.e = c->d_cph.as<uint64_t>();
        ph.nb = c->cph_nb;
        ph.WG = ct.WG;
        ph.gb = ct.gb;
        ph.rank_base = ct.rank_base;
        ph.flags = flags;
        ph.ep = c->cph_ep;
    }
    if (p.n)
        HIPCHK(c, compact_probes(p, c->ct, c->p_code_lo.as<uint64_t>(), c->p_code_hi.as<uint64_t>(), s, &ph));
    HIPCHK(c, launch_locate_c(ct, wt, p, c->p_code_lo.as<uint64_t>(), c->p_code_hi.as<uint64_t>(),
                              work, flags, s));
    HIPCHK_RC(c, t.mark(1));
    if (p.n && ct.ntiles) {
        // verdict bytes and bitmap from the plan and the join, as probe_ntiles
        const bool delta = pack_after_delta(c);
        work.bitmap = delta ? nullptr : b->bitmap;
        HIPCHK(c, launch_plan_s(work, ct.ntiles, c->w_items.as<uint32_t>(), s, flags,
                                (uint32_t)b->n_txn, b->verdict));
        HIPCHK_RC(c, t.mark(3));  // (no scatter)
        HIPCHK(c, launch_join_c(ct, work, max_items, b->verdict, s));
        HIPCHK_RC(c, tail_verdict(c, t, b, delta));
    } else {
        HIPCHK_RC(c, tail_flags(c, t, b, flags));
    }
#ifdef HSC_STAMPS
    HIPCHK_RC(c, stamp_report(c, work, max_items, 2, 7));
#endif
    return HSC_OK;
}

// The tile pipeline: locate -> plan -> scatter -> join -> pack.  (A caller's
// bound mapping runs after its own mark(0): it counts as locate time.)
int probe_tiles(hsc_ctx *c, const hsc_probe_batch *b, const WinView &w, const ProbeView &p,
                PhaseMarker &t)
{
    hipStream_t s = c->stream;
    c->probe_ntiles = w.ntiles;
    c->probe_buckets = false;
    const uint32_t nt = std::max<uint32_t>(w.ntiles, 1);
    ProbeWork work{};
    work.lds_mode = w.ntiles <= (uint32_t)kHistCap;
    const size_t nwork = std::max<size_t>(p.n, p.n_lock);
    work.G = (uint32_t)std::min<size_t>(kMaxChunks, std::max<size_t>(1, (nwork + 2047) / 2048));
    work.chunk = (uint32_t)((p.n + work.G - 1) / work.G);
    HIPCHK(c, c->w_code.ensure(8 * (size_t)std::max<uint32_t>(p.n, 1)));
    HIPCHK(c, c->w_hist.ensure(4 * (size_t)work.G * nt));
    HIPCHK(c, c->w_counts.ensure(4 * ((size_t)nt + 1)));
    HIPCHK(c, c->w_bucket.ensure(4 * ((size_t)nt + 1)));
    HIPCHK(c, c->w_cursor.ensure(4 * ((size_t)nt + 1)));
    HIPCHK(c, c->w_items.ensure(4 * ((size_t)nt + 1)));
    HIPCHK(c, c->w_recs.ensure(8 * (size_t)rec_words(w.W) * 2 * std::max<uint32_t>(p.n, 1)));
    const uint32_t max_items = nt + (uint32_t)((2 * (size_t)p.n + kJoinChunk - 1) / kJoinChunk);
    HIPCHK(c, c->w_item_tile.ensure(4 * (size_t)max_items + 16));
    HIPCHK(c, c->w_item_desc.ensure(16 * (size_t)max_items + 16));
    work.item_desc = c->w_item_desc.as<uint4>();
    work.code = c->w_code.as<uint64_t>();
    work.hist = c->w_hist.as<uint32_t>();
    work.counts = c->w_counts.as<uint32_t>();
    work.bucket_off = c->w_bucket.as<uint32_t>();
    work.cursor = c->w_cursor.as<uint32_t>();
    work.item_off = c->w_items.as<uint32_t>();
    work.item_tile = c->w_item_tile.as<uint32_t>();
    work.recs = c->w_recs.as<uint64_t>();
    HIPCHK_RC(c, t.mark(0));
    if (b->n_txn) HIPCHK(c, hipMemsetAsync(b->verdict, 0, b->n_txn, s));
    if (!work.lds_mode) HIPCHK(c, hipMemsetAsync(c->w_counts.p, 0, 4 * ((size_t)nt + 1), s));
    HIPCHK(c, launch_locate(w, p, work, b->verdict, s));
    HIPCHK_RC(c, t.mark(1));
    if (p.n && w.ntiles) {
        HIPCHK(c, launch_plan(w, work, s));
        HIPCHK_RC(c, t.mark(2));
        HIPCHK(c, launch_scatter(w, p, work, s));
        HIPCHK_RC(c, t.mark(3));
        HIPCHK(c, launch_join(w, work, max_items, b->verdict, s));
    }
    HIPCHK_RC(c, t.mark(4));
    HIPCHK_RC(c, probe_delta(c, b->verdict));
    HIPCHK(c, launch_pack(b->verdict, (uint32_t)b->n_txn, b->bitmap, s));
    return t.mark(5);
}

// Wide keys as compact codes: map the bounds, then the tile pipeline.
int probe_ccodes(hsc_ctx *c, const hsc_probe_batch *b, const WinView &w, const ProbeView &p,
                 PhaseMarker &t)
{
    const size_t n = std::max<uint32_t>(p.n, 1);
    HIPCHK(c, c->p_code_lo.ensure(8 * (size_t)c->ct.WC * n));
    HIPCHK(c, c->p_code_hi.ensure(8 * (size_t)c->ct.WC * n));
    HIPCHK_RC(c, t.mark(0));
    HIPCHK(c, compact_probes(p, c->ct, c->p_code_lo.as<uint64_t>(), c->p_code_hi.as<uint64_t>(),
                             c->stream));
    ProbeView pc = p;
    pc.lo = c->p_code_lo.as<uint64_t>();
    pc.hi = c->p_code_hi.as<uint64_t>();
    WinView wc = with_tables(c->wc, w);
    wc.gbits = w.gbits;
    return probe_tiles(c, b, wc, pc, t);
}

// A dense batch on a narrow window whose tile rows do not fit 8 bytes (or
// HSC_LAYOUT_NARROW_CODES): map the bounds to codes, all of group 0, then the
// tile pipeline over the one-word code rows.
int probe_ncodes(hsc_ctx *c, const hsc_probe_batch *b, const WinView &wn, const ProbeView &p,
                 PhaseMarker &t)
{
    const size_t n = std::max<uint32_t>(p.n, 1);
    HIPCHK(c, c->p_code_lo.ensure(8 * n));
    HIPCHK(c, c->p_code_hi.ensure(8 * n));
    const size_t zb = c->p_zero.bytes;
    HIPCHK(c, c->p_zero.ensure(4 * n));
    if (c->p_zero.bytes != zb) HIPCHK(c, hipMemsetAsync(c->p_zero.p, 0, c->p_zero.bytes, c->stream));
    HIPCHK_RC(c, t.mark(0));
    HIPCHK(c, narrow_codes(c->nv, p, c->p_code_lo.as<uint64_t>(), c->p_code_hi.as<uint64_t>(),
                           c->stream));
    ProbeView pn = p;
    pn.lo = c->p_code_lo.as<uint64_t>();
    pn.hi = c->p_code_hi.as<uint64_t>();
    pn.gid = c->p_zero.as<uint32_t>();
    return probe_tiles(c, b, wn, pn, t);
}

int probe_lane(hsc_ctx *c, const hsc_probe_batch *b)
{
    const WinView w = win_view(c);
    if (b->n > 0xFFFFFFFFull / 2 || b->n_lock > 0xFFFFFFFFull || b->n_txn > 0xFFFFFFFFull)
        return ctx_fail(c, HSC_EINVAL, "batch too large");
    ProbeView p = batch_view(*b);
    if (!w.n) p.n = 0;  // empty key window: no range can match
    c->raw_probe = p;
    c->raw_probe.n = (uint32_t)b->n;  // the delta may hold keys of an empty main window
    PhaseMarker t(c);
    const size_t nwork = std::max<size_t>(p.n, p.n_lock);
    // compact tiles for dense batches; a sparse one (fewer than kDirectPerTile
    // ranges per tile) takes the wide pipeline, which stages only the tiles
    // its ranges reach (the compact-tile join stages every tile)
    const bool compact_tiles =
        !c->narrow && c->compact && c->ctiles && c->layout != HSC_LAYOUT_COMPACT_WIDE &&
        p.n < (1u << 30) && b->n_txn < (1u << 30) && (size_t)p.n >= kDirectPerTile * (size_t)c->ctv.ntiles &&
        (nwork + ctiles_chunk() - 1) / ctiles_chunk() <= (size_t)kMaxChunks;
    // wide keys as compact codes through the tile pipeline
    const bool compact_codes = !c->narrow && c->compact;
    // narrow window: a sparse batch is answered by the direct probe; a dense
    // one maps its bounds to codes and runs the tile pipeline on the codes
    const bool direct = c->layout == HSC_LAYOUT_NARROW_DIRECT ||
                        (c->layout != HSC_LAYOUT_NARROW_TILES &&
                         (size_t)p.n < kDirectPerTile * (size_t)c->wn.ntiles);
    // 8-byte tile rows when they fit and the batch fits one column scan
    const bool narrow_tiles = c->ntiles32 && c->layout != HSC_LAYOUT_NARROW_CODES &&
                              (nwork + narrow_tiles_chunk() - 1) / narrow_tiles_chunk() <= (size_t)kMaxChunks;
    if (compact_tiles) return probe_ctiles(c, b, w, p, t);
    if (compact_codes) return probe_ccodes(c, b, w, p, t);
    if (!c->narrow) return probe_tiles(c, b, w, p, t);
    if (direct) return probe_narrow(c, b, w, p, t);
    if (narrow_tiles) return probe_ntiles(c, b, with_tables(c->wn, w), p, t);
    return probe_ncodes(c, b, with_tables(c->wn, w), p, t);
}

}  // namespace

int hsc::ctx_probe(hsc_ctx *c, const hsc_probe_batch *b)
{
    if (c->host_only) return ctx_fail(c, HSC_EDEVICE, "host-only context");
    if (c->pend_n || c->pend_t) HIPCHK_RC(c, ctx_flush_appends(c));  // the pending tail is k_small_narrow's only
    HIPCHK(c, select_lane(c));
    const int rc = probe_lane(c, b);
    // the lane's done event fences whatever probe_lane launched, also when it
    // failed part way: a later take-over of the lane or a window rebuild from
    // another stream waits on it before touching the lane's scratch; it is
    // recorded when the context leaves this stream (ctx_switch_stream)
    lane_mark(c);
    return rc;
}

int hsc::collect_timing(hsc_ctx *c)
{
    if (!c->timing || !c->ev[5]) return HSC_OK;
    HIPCHK(c, hipEventSynchronize(c->ev[5]));
    float t[5];
    for (int i = 0; i < 5; ++i) (void)hipEventElapsedTime(&t[i], c->ev[i], c->ev[i + 1]);
    c->last.locate_ms = t[0];
    c->last.plan_ms = t[1];
    c->last.scatter_ms = t[2];
    c->last.join_ms = t[3];
    c->last.pack_ms = t[4];
    (void)hipEventElapsedTime(&c->last.probe_total_ms, c->ev[0], c->ev[5]);
    uint64_t nrec = 0;
    if (c->probe_ntiles && c->w_counts.p && c->probe_buckets) {  // per-tile record counts
        std::vector<uint32_t> cnt(c->probe_ntiles);
        HIPCHK(c, hipMemcpy(cnt.data(), c->w_counts.p, 4 * cnt.size(), hipMemcpyDeviceToHost));
        for (uint32_t v : cnt) nrec += v;
    } else if (c->probe_ntiles && c->w_bucket.p) {
        uint32_t r = 0;
        HIPCHK(c, hipMemcpy(&r, c->w_bucket.as<uint32_t>() + c->probe_ntiles, 4, hipMemcpyDeviceToHost));
        nrec = r;
    }
    c->last.records = nrec;
    c->last.tiles = c->probe_ntiles;  // tiles of the view the last probe joined over
    return HSC_OK;
}
