// gw2_emu.cpp -- TEST-ONLY: the write loop's two-lookup schedule (k_gw_lane, loop 2) on the CPU.
// One lane walks a whole scan from bit 0 with icx_spec_core.h's write_step -- and, in the
// two-lookup schedule, write_step_more for a second AC lookup of the same block whenever the block
// did not end and the reader's window needs no refill -- with the kernels' error-byte bounds
// (ErrBounds) on every lookup. tests/test_gw2_emu.py requires both schedules to give the same
// blocks, DC values, block count, failing block and final bit position, and reads the study's
// counters (lookups, iterations, second lookups refused for block end / for bits).
// Never linked into libicx.so.
#include "spec_emu.cpp"  // emu_unstuff (the unstuff pass as the kernels compute it)

namespace {
struct Gw2Walk {
    int16_t* coef;
    int32_t* dc;
    int64_t bi = 0;
    int32_t pred[3] = {0, 0, 0};
    int ci = 0;
    void store(const WriteOut& o, bool dcl) {
        if (dcl) {
            pred[ci] = wadd(pred[ci], o.v1);
            dc[bi] = pred[ci];
        } else if (o.w1) {
            coef[bi * 64 + nat_of_zig(o.c1 & 63)] = (int16_t)o.v1;
        }
        if (o.w2) coef[bi * 64 + nat_of_zig(o.c2 & 63)] = (int16_t)o.v2;
    }
};
}  // namespace

extern "C" {
// two != 0: the two-lookup schedule; 0: write_step alone. coef: blocks x 64 int16 in natural order,
// dc: absolute DC values. out[0] blocks completed, [1] the failing block (-1: none), [2] final bit
// position, [3] lookups, [4] iterations, [5] second lookups refused because the block ended, [6]
// refused because the window held <= 32 bits, [7] second lookups before which a refill would have
// changed the reader (must be 0: write_step_more does not refill), [8] total blocks of the frame,
// [9] the failing lookup's position (1 first, 2 second; 0: none), [10] blocks that ended at a
// second lookup, [11] / [12] second lookups whose code was longer than the AC window: from the
// pool / by the canonical walk.
// Returns 0, or 2 for a stream the guess-write path does not take.
int gw2_walk(const uint8_t* file, int64_t size, int two, int16_t* coef, int32_t* dc, int64_t cap_blocks, int64_t* out) {
    auto dp = std::make_unique<Desc>();
    Desc& d = *dp;
    (void)parse_headers(file, size, d);
    const int64_t scan_len = d.size - d.scan_off;
    if (!(d.status == kPending && d.restart == 0 && d.nc >= 1 && d.bpm <= kSpecMaxBpm && scan_len > 0)) return 2;
    const int64_t total = (int64_t)d.mbw * d.mbh * d.bpm;
    if (total > cap_blocks) return 2;
    const uint8_t* R = file + d.scan_off;
    std::vector<uint8_t> U;
    int64_t errpos;
    int32_t giveup = 0;
    const int64_t ulen = emu_unstuff(R, scan_len, ustf_align(R), U, errpos, giveup, nullptr);
    if (giveup) return 2;
    auto SSp = std::make_unique<StepSet>();
    for (int k = 0; k < WriteTab::entries(); ++k) SSp->write.fill(d.huff, k);
    const Sel SL = make_sel(d);
    set_block_sel(SSp->write, d.huff, SL);
    const WriteTab& TW = SSp->write;
    const Huff* H = d.huff;
    std::memset(coef, 0, sizeof(int16_t) * 64 * total);
    std::memset(dc, 0, sizeof(int32_t) * total);
    Reader r;
    r.init(U.data(), ulen, 0);
    ErrBounds eb;
    eb.set(errpos == INT64_MAX ? INT64_MAX : errpos * 8, 0);
    Gw2Walk w{coef, dc};
    int b = 0, z = 0;
    int64_t lookups = 0, iters = 0, by_end = 0, by_bits = 0, refill_moved = 0, errblk = -1, errpos2 = 0, end2 = 0, pool2 = 0,
            walk2 = 0;
    while (w.bi < total) {  // one iteration of k_gw_lane's write loop, one lane
        ++iters;
        const bool dcl = z == 0;
        if (dcl) w.ci = SL.comp(b);
        const uint32_t u0 = r.used;
        const WriteOut o = write_step(r, TW, H, SL, b, z, eb.near(u0));
        ++lookups;
        if (eb.fail(u0, o.err, r.used)) { errblk = w.bi; errpos2 = 1; break; }
        w.store(o, dcl);
        if (two) {
            if (z == 0) {
                ++by_end;
            } else if (r.nb <= 32) {
                ++by_bits;
            } else {
                {  // the refill write_step_more leaves out is a no-op here
                    Reader q = r;
                    q.refill();
                    refill_moved += q.buf != r.buf || q.nb != r.nb || q.na != r.na || q.a0 != r.a0 || q.a1 != r.a1;
                }
                const uint32_t e1 = TW.look_b(b, false, (uint32_t)(r.buf >> 32));
                pool2 += (e1 & kStSlow) == kStSub;
                walk2 += (e1 & kStSearch) != 0;
                const uint32_t u1 = r.used;
                const WriteOut o2 = write_step_more(r, TW, H, SL, b, z, eb.near(u1));
                ++lookups;
                if (eb.fail(u1, o2.err, r.used)) { errblk = w.bi; errpos2 = 2; break; }
                w.store(o2, false);
                end2 += z == 0;
            }
        }
        if (z == 0) ++w.bi;
    }
    out[0] = w.bi; out[1] = errblk; out[2] = r.pos(); out[3] = lookups; out[4] = iters; out[5] = by_end;
    out[6] = by_bits; out[7] = refill_moved; out[8] = total; out[9] = errpos2; out[10] = end2; out[11] = pool2;
    out[12] = walk2;
    return 0;
}

// gw_lane_err on a lane given by its records' (b, cnt) pairs, its GwOut::err and its count record
// (m, c, err): the lane-relative block of the first true-path failure (INT32_MAX: none).
int32_t gw2_lane_err(const int32_t* rec_b, const int32_t* rec_cnt, int nrec, int32_t gerr, int32_t cm, int32_t cc,
                     int32_t cerr) {
    RecState rec[kRec];
    std::memset(rec, 0, sizeof rec);
    GwOut g{};
    for (int i = 0; i < nrec && i < kRec; ++i) {
        rec[i].b = rec_b[i];
        rec[i].cnt = rec_cnt[i];
        g.rerr |= rec_b[i] != 0;  // (as k_gw_lane sets it)
    }
    g.nrec = nrec;
    g.err = gerr;
    GcRec c{};
    c.m = cm;
    c.c = cc;
    c.err = cerr;
    return gw_lane_err(g, c, rec);
}
}
