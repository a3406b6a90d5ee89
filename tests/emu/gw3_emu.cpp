// gw3_emu.cpp -- TEST-ONLY: the write loop's second lookup on a partly filled window (k_gw_lane,
// loop 2, the instance without error-byte bounds) on the CPU. One lane walks a whole scan from bit 0
// as gw2_walk does, but the second lookup of an iteration is icx_spec_core.h's write_step_short:
// taken when the block did not end and either the window holds more than 32 bits or the first-level
// entry at the zero-padded peek is a plain one whose symbols fit the nb valid bits. The walk counts
// the lookups, the iterations, the short lookups committed and the refusals by cause, and checks
// that a refused lane is left untouched. Like gw2_walk it tests the error-byte bounds (ErrBounds) on
// every lookup, so one walk also serves streams that end in a syntax error (the kernel's instance
// for those keeps full windows; the bounds see the same symbol starts either way).
// tests/test_gw3_emu.py compares it with gw2_walk's schedules and the oracle's trace. Never linked
// into libicx.so.
#include "gw2_emu.cpp"

extern "C" {
// coef / dc as gw2_walk. out[0] blocks completed, [1] the failing block (-1: none), [2] final bit
// position, [3] lookups, [4] iterations, [5] second lookups refused because the block ended, [6]
// refused for a slow (SUB / SEARCH) or error entry on a window of <= 32 bits, [7] refused because
// the entry's symbols take more than the nb bits the window holds, [8] total blocks of the frame,
// [9] the failing lookup's position (1 first, 2 second; 0: none), [10] blocks that ended at a second
// lookup, [11] short lookups committed (second lookups out of a window of <= 32 bits), [12] those
// that left the window empty (nb == 0), [13] refused lookups that changed the reader, the state or
// the output (must be 0), [14] committed lookups that consumed more than nb bits (must be 0), [15]
// those of [7] whose first symbol alone would have fit (a pair whose second symbol does not).
// Returns 0, or 2 for a stream the guess-write path does not take.
int gw3_walk(const uint8_t* file, int64_t size, int16_t* coef, int32_t* dc, int64_t cap_blocks, int64_t* out) {
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
    int64_t lookups = 0, iters = 0, by_end = 0, by_entry = 0, by_fit = 0, errblk = -1, errpos2 = 0, end2 = 0, shorts = 0,
            emptied = 0, touched = 0, overran = 0, fit_pair = 0;
    while (w.bi < total) {  // one iteration of k_gw_lane's write loop, one lane
        ++iters;
        const bool dcl = z == 0;
        if (dcl) w.ci = SL.comp(b);
        const uint32_t u0 = r.used;
        const WriteOut o = write_step(r, TW, H, SL, b, z, eb.near(u0));
        ++lookups;
        if (eb.fail(u0, o.err, r.used)) { errblk = w.bi; errpos2 = 1; break; }
        w.store(o, dcl);
        if (z == 0) {
            ++by_end;
        } else {
            const Reader q = r;
            const int b0 = b, z0 = z;
            const uint32_t e1 = TW.look_b(b, false, (uint32_t)(r.buf >> 32));
            WriteOut o2;
            std::memset(&o2, 0x5a, sizeof o2);
            const uint32_t u1 = r.used;
            if (write_step_short(r, TW, H, SL, b, z, eb.near(u1), o2)) {
                ++lookups;
                const bool sh = q.nb <= 32;
                shorts += sh;
                emptied += sh && r.nb == 0;
                overran += r.nb < 0 || (int)(r.used - u1) > q.nb;
                if (eb.fail(u1, o2.err, r.used)) { errblk = w.bi; errpos2 = 2; break; }
                w.store(o2, false);
                end2 += z == 0;
            } else {
                const int32_t kMark = 0x5a5a5a5a;
                touched += q.buf != r.buf || q.nb != r.nb || q.na != r.na || q.a0 != r.a0 || q.a1 != r.a1 || q.used != r.used ||
                           q.tick != r.tick || q.hb != r.hb || q.next != r.next || b != b0 || z != z0;
                touched += o2.v1 != kMark || o2.v2 != kMark || o2.c1 != kMark || o2.c2 != kMark || o2.n1 != kMark || o2.n2 != kMark;
                touched += q.nb > 32;  // (a full window is never refused)
                if ((e1 & (kStSlow | kStErr1)) != 0u) {
                    ++by_entry;
                } else {
                    ++by_fit;
                    fit_pair += (int)st_tot1(e1) <= q.nb;  // (symbol 1 fits, the pair does not)
                }
            }
        }
        if (z == 0) ++w.bi;
    }
    out[0] = w.bi; out[1] = errblk; out[2] = r.pos(); out[3] = lookups; out[4] = iters; out[5] = by_end;
    out[6] = by_entry; out[7] = by_fit; out[8] = total; out[9] = errpos2; out[10] = end2; out[11] = shorts;
    out[12] = emptied; out[13] = touched; out[14] = overran; out[15] = fit_pair;
    return 0;
}
}
