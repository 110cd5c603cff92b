// kdtn_qplan.h — MakeQdiscs for one message's own property strings: the twelve strings parsed
// where they lie (an LDS window or the stream) and the qdisc record composed from the values.
// One copy for the planners that work from request bodies: k_rp_plan (kdtn_remote.hip) and
// k_ul_plan (kdtn_update.hip).
#pragma once
#include "kdtn_wirewalk.h"

namespace kdtn {

// The twelve property strings parsed where they lie: what k_pdict_parse leaves in the parsed
// tables for the same bytes ("" parses to 0 everywhere), and the columns that failed.
struct RpVals {
    uint32_t v[KDTN_NPROP];          // duration µs, Percentage2u32, the rate's low word
    uint32_t lat_t, jit_t, rate_hi;  // time2Tick of the two durations, the rate's high word
    uint32_t bad;                    // bit k: column k failed to parse
};

// The non-empty strings among (po[k], pl[k]), k = KDTN_P_*, parsed into pv (zeroed by the
// caller). at(off) gives the bytes of stream offset off. One loop with three call sites, not twelve: the parsers are large.
template <typename At>
KD_INLINE void props_parse(const At& at, const uint32_t* po, const uint32_t* pl, double tick, RpVals& pv) {
#pragma unroll 1
    for (uint32_t k = 0; k < (uint32_t)KDTN_NPROP; ++k) {
        uint32_t off = 0, len = 0;
#pragma unroll
        for (int j = 0; j < KDTN_NPROP; ++j) {
            off = k == (uint32_t)j ? po[j] : off;
            len = k == (uint32_t)j ? pl[j] : len;
        }
        if (!len) continue;
        const uint8_t* s = at(off);
        uint32_t x = 0, y = 0;
        bool ok;
        if (k == KDTN_P_LATENCY || k == KDTN_P_JITTER) {
            ok = parse_duration_us(s, len, &x);
            y = time2tick(x, tick);
        } else if (k == KDTN_P_RATE) {
            uint64_t r = 0;
            ok = parse_rate(s, len, &r);
            x = (uint32_t)r;
            y = (uint32_t)(r >> 32);
        } else {
            float pct = 0.f;
            ok = parse_pct(s, len, &pct);
            x = ok ? p2u(pct) : 0u;
        }
        if (!ok) {
            x = y = 0;
            pv.bad |= 1u << k;
        }
#pragma unroll
        for (int j = 0; j < KDTN_NPROP; ++j) pv.v[j] = k == (uint32_t)j ? x : pv.v[j];
        pv.lat_t = k == KDTN_P_LATENCY ? y : pv.lat_t;
        pv.jit_t = k == KDTN_P_JITTER ? y : pv.jit_t;
        pv.rate_hi = k == KDTN_P_RATE ? y : pv.rate_hi;
    }
}

// MakeQdiscs over parsed values: qdisc_from's sibling (same error order, NewNetem conditionals
// and TBF burst; common/qdisc.go:20-126 + netlink NewNetem), for values parsed per message
// instead of gathered from the dictionary tables.
KD_INLINE void qdisc_from_parsed(const RpVals& p, uint32_t gap, bool empty, uint32_t* q) {
#pragma unroll
    for (int w = 0; w < 18; ++w) q[w] = 0;
    if (empty) return;
    if (p.bad) {
        // reference order: columns 0-4, then 6-11, the rate (5) last = KDTN_E_LATENCY … KDTN_E_RATE
        const uint32_t ord = (p.bad & 0x1Fu) | ((p.bad >> 6) << 5) | (((p.bad >> 5) & 1u) << 11);
        q[17] = ((uint32_t)KDTN_E_LATENCY + (uint32_t)__builtin_ctz(ord)) << 16;   // byte 70 = err
        return;
    }
    const uint32_t lat_us = p.v[KDTN_P_LATENCY], jit_us = p.v[KDTN_P_JITTER];
    const uint32_t los = p.v[KDTN_P_LOSS], dup = p.v[KDTN_P_DUPLICATE], rop = p.v[KDTN_P_REORDER_PROB];
    q[0] = p.lat_t;                                                     // latency
    q[1] = (lat_us > 0 && jit_us > 0) ? p.v[KDTN_P_LATENCY_CORR] : 0u;  // delay_corr
    q[2] = 1000u;                                                       // limit
    q[3] = los;                                                         // loss
    q[4] = los > 0 ? p.v[KDTN_P_LOSS_CORR] : 0u;                        // loss_corr
    q[5] = (rop > 0 && gap == 0) ? 1u : gap;                            // gap
    q[6] = dup;                                                         // duplicate
    q[7] = dup > 0 ? p.v[KDTN_P_DUPLICATE_CORR] : 0u;                   // duplicate_corr
    q[8] = p.lat_t > 0 ? p.jit_t : jit_us;                              // jitter
    q[9] = rop;
    q[10] = p.v[KDTN_P_REORDER_CORR];
    q[11] = p.v[KDTN_P_CORRUPT_PROB];
    q[12] = p.v[KDTN_P_CORRUPT_CORR];
    const uint64_t rate = ((uint64_t)p.rate_hi << 32) | p.v[KDTN_P_RATE];
    uint32_t has_tbf = 0;
    if (rate != 0) {
        uint32_t burst = (uint32_t)(rate / 250ull);                     // getTbfBurst
        if (burst < 5000u) burst = 5000u;
        q[13] = burst;
        q[14] = p.v[KDTN_P_RATE];
        q[15] = p.rate_hi;
        q[16] = 1500u;
        has_tbf = 1;
    }
    q[17] = 1u | (has_tbf << 8);                                        // has_netem, has_tbf, err = 0
}

// The plan of one message's properties at Q (18 dwords): MakeQdiscs(properties), the empty
// record when no string and no gap is set (absent properties, like nil). Returns its err.
template <typename At>
KD_INLINE uint32_t qdisc_plan(const At& at, const uint32_t* po, const uint32_t* pl, uint32_t gap, double tick, uint32_t* Q) {
    RpVals pv;
#pragma unroll
    for (int k = 0; k < KDTN_NPROP; ++k) pv.v[k] = 0;
    pv.lat_t = pv.jit_t = pv.rate_hi = pv.bad = 0;
    uint32_t any = gap;
#pragma unroll
    for (int k = 0; k < KDTN_NPROP; ++k) any |= pl[k];
    if (any) props_parse(at, po, pl, tick, pv);
    qdisc_from_parsed(pv, gap, any == 0, Q);
    return (Q[17] >> 16) & 0xFFu;
}

}  // namespace kdtn
