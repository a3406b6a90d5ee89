// gw4_emu.cpp -- TEST-ONLY: the write loop's further lookups with the cap as a parameter (k_gw_lane,
// loop 2, the instance without error-byte bounds) on the CPU. One lane walks a whole scan from bit 0
// as gw3_walk does: write_step, then icx_spec_core.h's write_step_short again and again while it is
// taken and the block goes on, up to `cap` lookups per iteration (2: gw3_walk's schedule; 3: the
// kernel's). The walk counts, by the position of the lookup in its iteration, the lookups taken,
// the refusals by cause, the blocks that end there, the windows left empty and the pairs committed,
// and checks that a refused lane is left untouched and that no lookup consumes more than the
// window holds. Like gw3_walk it tests the error-byte bounds (ErrBounds) on every lookup.
// tests/test_gw4_emu.py compares the caps with each other and with the oracle's trace. Never linked
// into libicx.so.
#include "gw3_emu.cpp"

extern "C" {
// coef / dc as gw2_walk. cap: lookups per iteration at most, 1 .. kGw4MaxCap.
// out[0] blocks completed, [1] the failing block (-1: none), [2] final bit position, [3] lookups,
// [4] iterations, [5] total blocks of the frame, [6] the failing lookup's position (0: none), [7]
// refused lookups that changed the reader, the state or the output (must be 0), [8] committed
// lookups that consumed more than nb bits or left nb < 0 (must be 0).
// Then eight counters per position p = 1 .. kGw4MaxCap at out[16 + 8 * (p - 1)]: [0] lookups taken
// at p, [1] refused because the block had ended, [2] refused for a slow (SUB / SEARCH) or error entry
// on a window of <= 32 bits, [3] refused because the entry's symbols take more than the nb bits the
// window holds, [4] blocks that ended at p, [5] lookups out of a window of <= 32 bits that left it
// empty (nb == 0), [6] pairs committed at p (both symbols written), [7] those of [2] whose entry was
// an invalid code (it waits for the next iteration's full window).
// Returns 0, or 2 for a stream the guess-write path does not take, or 3 for a cap out of range.
enum { kGw4MaxCap = 8, kGw4Out = 16 + 8 * kGw4MaxCap };
int gw4_walk(const uint8_t* file, int64_t size, int cap, int16_t* coef, int32_t* dc, int64_t cap_blocks, int64_t* out) {
    if (cap < 1 || cap > kGw4MaxCap) return 3;
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
    std::memset(out, 0, sizeof(int64_t) * kGw4Out);
    Reader r;
    r.init(U.data(), ulen, 0);
    ErrBounds eb;
    eb.set(errpos == INT64_MAX ? INT64_MAX : errpos * 8, 0);
    Gw2Walk w{coef, dc};
    int b = 0, z = 0;
    int64_t lookups = 0, iters = 0, errblk = -1, errat = 0, touched = 0, overran = 0;
    auto at = [&](int p, int c) -> int64_t& { return out[16 + 8 * (p - 1) + c]; };
    while (w.bi < total && errat == 0) {  // one iteration of k_gw_lane's write loop, one lane
        ++iters;
        const bool dcl = z == 0;
        if (dcl) w.ci = SL.comp(b);
        const uint32_t u0 = r.used;
        const WriteOut o = write_step(r, TW, H, SL, b, z, eb.near(u0));
        ++lookups;
        ++at(1, 0);
        if (eb.fail(u0, o.err, r.used)) { errblk = w.bi; errat = 1; break; }
        w.store(o, dcl);
        at(1, 4) += z == 0;
        at(1, 6) += o.w2;
        for (int p = 2; p <= cap; ++p) {
            if (z == 0) { ++at(p, 1); break; }
            const Reader q = r;
            const int b0 = b, z0 = z;
            const uint32_t e1 = TW.look_b(b, false, (uint32_t)(r.buf >> 32));
            WriteOut o2;
            std::memset(&o2, 0x5a, sizeof o2);
            const uint32_t u1 = r.used;
            if (!write_step_short(r, TW, H, SL, b, z, eb.near(u1), o2)) {
                const int32_t kMark = 0x5a5a5a5a;
                touched += q.buf != r.buf || q.nb != r.nb || q.na != r.na || q.a0 != r.a0 || q.a1 != r.a1 || q.used != r.used ||
                           q.tick != r.tick || q.hb != r.hb || q.next != r.next || b != b0 || z != z0;
                touched += o2.v1 != kMark || o2.v2 != kMark || o2.c1 != kMark || o2.c2 != kMark || o2.n1 != kMark || o2.n2 != kMark;
                touched += q.nb > 32;  // (a full window is never refused)
                if ((e1 & (kStSlow | kStErr1)) != 0u) {
                    ++at(p, 2);
                    at(p, 7) += (e1 & kStSlow) == 0u;
                } else {
                    ++at(p, 3);
                }
                break;
            }
            ++lookups;
            ++at(p, 0);
            overran += r.nb < 0 || (int)(r.used - u1) > q.nb;
            at(p, 5) += q.nb <= 32 && r.nb == 0;
            if (eb.fail(u1, o2.err, r.used)) { errblk = w.bi; errat = p; break; }
            w.store(o2, false);
            at(p, 4) += z == 0;
            at(p, 6) += o2.w2;
        }
        if (errat == 0 && z == 0) ++w.bi;
    }
    out[0] = w.bi; out[1] = errblk; out[2] = r.pos(); out[3] = lookups; out[4] = iters; out[5] = total;
    out[6] = errat; out[7] = touched; out[8] = overran;
    return 0;
}
}
