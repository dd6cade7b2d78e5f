/* LDS bank-conflict model of k_lz_walk (development aid, not product, not oracle).
 * Replays the walk of oracle E wavefront by wavefront in lock step, as the kernel runs it (a walker of LPW lanes per range,
 * 64 / LPW walkers a wavefront, ranges taken in order), collects every LDS read address per access site and prices each
 * wave-instruction with the bank rules of MI355X_MICROARCH.md §LDS:
 *   ds_read_b32  : groups {0-31}, {32-63}; bank = (a / 4) mod 32; cycles = sum over groups of max(1, most distinct dwords on a bank)
 *   ds_read_b64  : same groups; bank pair = (a / 8) mod 32
 *   ds_read_b128 : 4 groups of 16 lanes; slot = (a / 16) mod 16
 * Variants: idle lanes reading (the round-3 kernel) or masked, the source rows skewed (addr = p + PAD * (p >> 8)),
 * dword reads or 8-byte-aligned reads.
 * build + run: tools/lab/ldssim.py */
#include <stdio.h>
#include "../../oracle/zso_encoder.c"

enum { S_REPA, S_REPB, S_REPC, S_DIST, S_SCA, S_SCB, S_EXA, S_EXB, NSITE };
static const char *siteName[NSITE] = { "rep a", "rep b", "rep c", "dist u16", "score a", "score b", "extend a", "extend b" };
enum { V_ALL32, V_MASK32, V_MASK32_SKEW, V_MASK64, V_MASK64_SKEW, V_MASK64_SKEW_PAIR, NVAR };
static const char *varName[NVAR] = { "b32 all lanes", "b32 idle masked", "b32 masked+skew", "b64 masked", "b64 masked+skew", "b64 m+s, pair-shared" };
static double cyc[NVAR][NSITE], ins[NVAR][NSITE];
static unsigned long long waveSteps, laneStepsActive, laneStepsAll, extRounds;
static int PAD = 24, LPW = 2;
#define SRC_BASE 8224u   /* LDS address of source byte 0 in the 64 KiB kernel */

static U32 skew(U32 p, int on) { return SRC_BASE + p + (on ? (U32)PAD * (p >> 8) : 0u); }

/* cost of one wave instruction: addr[lane] (byte address, already aligned to `width`), act[lane] */
static U32 costInstr(const U32 *addr, const unsigned char *act, int width)
{
    U32 total = 0;
    if (width == 16) {
        static const unsigned char grp[4][16] = { { 0,1,2,3,12,13,14,15,20,21,22,23,24,25,26,27 }, { 4,5,6,7,8,9,10,11,16,17,18,19,28,29,30,31 },
                                                  { 32,33,34,35,44,45,46,47,52,53,54,55,56,57,58,59 }, { 36,37,38,39,40,41,42,43,48,49,50,51,60,61,62,63 } };
        for (int g = 0; g < 4; g++) {
            U32 seen[16][16], cnt[16] = { 0 }, mx = 1;
            for (int i = 0; i < 16; i++) { int l = grp[g][i]; if (!act[l]) continue; U32 a = addr[l] >> 4, b = a & 15u, k; for (k = 0; k < cnt[b]; k++) if (seen[b][k] == a) break; if (k == cnt[b]) { seen[b][cnt[b]++] = a; if (cnt[b] > mx) mx = cnt[b]; } }
            total += mx;
        }
        return total;
    }
    for (int g = 0; g < 2; g++) {
        U32 seen[32][32], cnt[32] = { 0 }, mx = 1;
        for (int i = 0; i < 32; i++) {
            int l = g * 32 + i; if (!act[l]) continue;
            U32 a = addr[l] / (U32)width, b = a & 31u, k;
            for (k = 0; k < cnt[b]; k++) if (seen[b][k] == a) break;
            if (k == cnt[b]) { seen[b][cnt[b]++] = a; if (cnt[b] > mx) mx = cnt[b]; }
        }
        total += mx;
    }
    return total;
}

/* a span of `bytes` bytes starting at source position p (may be negative relative: caller passes p >= 0 or handles), per lane */
typedef struct { U32 p[64]; unsigned char act[64], live[64]; } Span;   /* act: lane takes part logically; live: walker is walking */

static void priceSpan(int site, const Span *s, U32 bytes, const U32 *pairBase /* walker-level base position or NULL */)
{
    U32 a[64]; unsigned char on[64];
    int l;
    /* b32 variants: (bytes + 3) / 4 + 1 dwords from the aligned-down start: the kernel's lds_span<K> reads K + 1 */
    U32 const nd = (bytes + 3) / 4 + 1;
    for (int v = 0; v < NVAR; v++) {
        int const sk = (v == V_MASK32_SKEW || v == V_MASK64_SKEW || v == V_MASK64_SKEW_PAIR);
        int const w = (v >= V_MASK64) ? 8 : 4;
        for (l = 0; l < 64; l++) {
            U32 p = s->p[l];
            if (v == V_MASK64_SKEW_PAIR && pairBase) p = pairBase[l];
            a[l] = skew(p, sk) & ~(U32)(w - 1);
            on[l] = (v == V_ALL32) ? 1 : (s->live[l] && s->act[l]);
        }
        U32 n;
        if (w == 4) n = nd;
        else {
            /* 8-byte reads: enough to cover the worst start: (7 + bytes + 7) / 8 ; pair-shared reads cover the walker's whole stretch */
            U32 span = bytes;
            if (v == V_MASK64_SKEW_PAIR && pairBase) span = bytes + (U32)(LPW - 1) * 2u;   /* lanes RPL = 2 apart */
            n = (7 + span + 7) / 8;
        }
        U32 c = costInstr(a, on, w);
        cyc[v][site] += (double)c * n;    /* the following dwords shift every address by the same amount: same conflicts */
        ins[v][site] += n;
    }
}

typedef struct { U32 ip, anchor, rep0, rep1, scanEnd, limit, start, steps; int active; } Walker;

/* Park and re-pack, the ideal policy: a wavefront runs until at most T of its walkers are still walking, parks those (one step charged for
   the hand-over), and the unit's parked walkers are packed WPW to a wavefront, the longest together, each such wavefront running as long as its longest.
   Counted in wave steps against the lock-step walk as it is (waveSteps); moving the state is free here, so this bounds what re-packing can win. */
#define NPARK 6
static const U32 parkT[NPARK] = { 2, 4, 6, 8, 12, 16 };
static unsigned long long parkSteps[NPARK], rangeSteps, rangesWalked;
static int cmpDesc(const void *a, const void *b) { U32 const x = *(const U32 *)a, y = *(const U32 *)b; return (x < y) - (x > y); }
static void parkUnit(const U32 *steps, U32 nRanges, U32 WPW)
{
    static U32 rest[NPARK][1024];
    U32 nRest[NPARK] = { 0 };
    for (U32 r0 = 0; r0 < nRanges; r0 += WPW) {
        U32 s[64], nw = (nRanges - r0 < WPW) ? nRanges - r0 : WPW;
        memcpy(s, steps + r0, nw * sizeof(U32));
        qsort(s, nw, sizeof(U32), cmpDesc);
        for (int t = 0; t < NPARK; t++) {
            U32 const T = parkT[t], own = (nw > T) ? s[T] : 0;        /* the step after which at most T walk on */
            int parked = 0;
            for (U32 k = 0; k < T && k < nw; k++) if (s[k] > own) { rest[t][nRest[t]++] = s[k] - own; parked = 1; }
            parkSteps[t] += own + (parked ? 1u : 0u);
        }
    }
    for (int t = 0; t < NPARK; t++) {
        qsort(rest[t], nRest[t], sizeof(U32), cmpDesc);          /* the longest together: the packing that costs the fewest steps */
        for (U32 k = 0; k < nRest[t]; k += WPW) {
            U32 longest = 0;
            for (U32 j = k; j < k + WPW && j < nRest[t]; j++) if (rest[t][j] > longest) longest = rest[t][j];
            parkSteps[t] += longest;
        }
    }
}

static void simUnit(Work *w, const BYTE *src, U32 n, const EParams *prm)
{
    U32 const WS = 1u << prm->walkLog, nRanges = (n + WS - 1) >> prm->walkLog;
    U32 const WPW = 64u / (U32)LPW;                       /* walkers per wavefront */
    U32 const look = (U32)prm->look, repWin = (U32)prm->repWin, CPL = look / (U32)LPW, RPL = repWin / (U32)LPW;
    U32 const hashable = (n >= 8) ? n - 7 : 0;
    U32 stepsOf[1024];                                    /* walker steps of every range of the unit (a walker's steps do not depend on its neighbours) */
    findCandidates(w, src, n, prm, 0);
    for (U32 r0 = 0; r0 < nRanges; r0 += WPW) {
        Walker wk[32];
        U32 nw = (nRanges - r0 < WPW) ? nRanges - r0 : WPW, k;
        memset(wk, 0, sizeof wk);
        for (k = 0; k < nw; k++) {
            U32 const start = (r0 + k) << prm->walkLog, blockStart = start & ~(BLOCK_MAX - 1), blockEnd = blockStart + ((n - blockStart < BLOCK_MAX) ? n - blockStart : BLOCK_MAX);
            U32 const end = (start + WS < blockEnd) ? start + WS : blockEnd;
            wk[k].limit = (end + CROSS_MAX < blockEnd) ? end + CROSS_MAX : blockEnd;
            wk[k].scanEnd = (end < hashable) ? end : hashable;
            wk[k].ip = wk[k].anchor = wk[k].start = start; wk[k].active = wk[k].ip < wk[k].scanEnd;
        }
        for (;;) {
            int any = 0;
            for (k = 0; k < nw; k++) any |= wk[k].active;
            if (!any) break;
            waveSteps++;
            Span ra, rb, rc, sa[4], sb[4], dd[4];
            U32 pairA[64], pairB[64], pairC[64];
            U32 bq[32], boff[32], bfwd[32]; int took[32];
            memset(&ra, 0, sizeof ra); memset(&rb, 0, sizeof rb); memset(&rc, 0, sizeof rc); memset(sa, 0, sizeof sa); memset(sb, 0, sizeof sb); memset(dd, 0, sizeof dd);
            for (k = 0; k < WPW; k++) {
                Walker *W = &wk[k < nw ? k : 0];
                int const live = k < nw && W->active;
                U32 const ip = W->ip;
                laneStepsAll += (U32)LPW; if (live) { laneStepsActive += (U32)LPW; W->steps++; }
                int const t0 = live && W->rep0 && ip >= W->rep0, t1 = live && W->rep1 && ip >= W->rep1;
                for (U32 sub = 0; sub < (U32)LPW; sub++) {
                    U32 const l = k * (U32)LPW + sub, p0 = ip + sub * RPL;
                    ra.p[l] = p0; rb.p[l] = t0 ? p0 - W->rep0 : p0; rc.p[l] = t1 ? p0 - W->rep1 : p0;
                    pairA[l] = ip; pairB[l] = t0 ? ip - W->rep0 : ip; pairC[l] = t1 ? ip - W->rep1 : ip;
                    ra.act[l] = rb.act[l] = rc.act[l] = 1; ra.live[l] = rb.live[l] = rc.live[l] = (unsigned char)live;
                }
                /* the step of walkRange, keeping the candidates in order */
                U32 cq[8], coff[8], nc = 0;
                int bestGain = 0, have = 0; U32 bestQ = 0, bestFwd = 0, bestBack = 0, bestOff = 0, q;
                U32 const wend = ((ip & ~7u) + 8u * (U32)LPW < W->scanEnd) ? (ip & ~7u) + 8u * (U32)LPW : W->scanEnd;
                if (live) for (q = ip; q < wend && nc < look; q++) {
                    U32 off = 0, fwd, back = 0; int isRep = 0, gain;
                    if (q < ip + repWin && q + 4 <= W->limit) {
                        if (t0 && rd32(src + q) == rd32(src + q - W->rep0)) { off = W->rep0; isRep = 1; }
                        else if (t1 && rd32(src + q) == rd32(src + q - W->rep1)) { off = W->rep1; isRep = 1; }
                    }
                    if (!off) off = w->dist[q];
                    if (!off) continue;
                    cq[nc] = q; coff[nc] = off; nc++;
                    fwd = matchLen(src, q, q - off, W->limit);
                    if (fwd < (isRep ? REPMIN : MINMATCH)) continue;
                    while (back < BCAP && q - back > W->anchor && q - off - back > 0 && src[q - back - 1] == src[q - off - back - 1]) back++;
                    gain = (int)((fwd > FCAP ? FCAP : fwd) + back) * 4 - (isRep ? 0 : (int)highbit32(off + 1)) - 4 * ((int)(q - back) - (int)ip) - (int)(q - ip);
                    if (!have || gain > bestGain) { have = 1; bestGain = gain; bestQ = q; bestFwd = fwd; bestBack = back; bestOff = off; }
                }
                for (U32 sub = 0; sub < (U32)LPW; sub++) for (U32 c = 0; c < CPL; c++) {
                    U32 const l = k * (U32)LPW + sub, ci = sub * CPL + c;
                    int const hv = live && ci < nc;
                    U32 const qq = hv ? cq[ci] : ip, of = hv ? coff[ci] : 0;
                    sa[c].p[l] = qq - 4 + 0; sb[c].p[l] = qq - of - 4;          /* (front pad: positions < 4 read the pad) */
                    if (qq < 4) { sa[c].p[l] = 0; } if (qq - of < 4) sb[c].p[l] = 0;
                    sa[c].act[l] = sb[c].act[l] = (unsigned char)hv; sa[c].live[l] = sb[c].live[l] = (unsigned char)live;
                    /* the distance: lane slot of the exchange buffer */
                    dd[c].p[l] = ((k * (U32)LPW + ((qq >> 3) - (ip >> 3))) * 16u + (qq & 7u) * 2u);
                    dd[c].act[l] = (unsigned char)hv; dd[c].live[l] = (unsigned char)live;
                }
                took[k] = live && have; bq[k] = bestQ; boff[k] = bestOff; bfwd[k] = bestFwd;
                if (live) {
                    if (have) {
                        W->ip = bestQ + bestFwd; W->anchor = W->ip;
                        if (bestOff == W->rep1) { W->rep1 = W->rep0; W->rep0 = bestOff; } else if (bestOff != W->rep0) { W->rep1 = W->rep0; W->rep0 = bestOff; }
                    } else W->ip = wend;
                    if (W->ip >= W->scanEnd) W->active = 0;
                }
            }
            priceSpan(S_REPA, &ra, RPL + 3, pairA); priceSpan(S_REPB, &rb, RPL + 3, pairB); priceSpan(S_REPC, &rc, RPL + 3, pairC);
            for (U32 c = 0; c < CPL; c++) { priceSpan(S_SCA, &sa[c], 12, NULL); priceSpan(S_SCB, &sb[c], 12, NULL); }
            for (U32 c = 0; c < CPL; c++) {   /* dist: 2-byte reads from the exchange buffer (address 0 based, no skew) */
                U32 a[64]; unsigned char on[64];
                for (int v = 0; v < NVAR; v++) { for (int l = 0; l < 64; l++) { a[l] = dd[c].p[l] & ~3u; on[l] = v == V_ALL32 ? 1 : (dd[c].live[l]); } cyc[v][S_DIST] += costInstr(a, on, 4); ins[v][S_DIST] += 1; }
            }
            /* whole length: rounds of 16 bytes a lane */
            {
                U32 pos[32]; int need[32], anyNeed = 0;
                for (k = 0; k < WPW; k++) { need[k] = k < nw && took[k] && bfwd[k] >= FCAP && wk[k].limit - bq[k] > FCAP; pos[k] = bq[k] + FCAP; anyNeed |= need[k]; }
                while (anyNeed) {
                    Span ea, eb; memset(&ea, 0, sizeof ea); memset(&eb, 0, sizeof eb);
                    extRounds++;
                    anyNeed = 0;
                    for (k = 0; k < WPW; k++) for (U32 sub = 0; sub < (U32)LPW; sub++) {
                        U32 const l = k * (U32)LPW + sub, fo = 16u * sub;
                        int const on = need[k] && fo < wk[k].limit - pos[k];
                        ea.p[l] = on ? pos[k] + fo : 0; eb.p[l] = on ? pos[k] - boff[k] + fo : 0; ea.act[l] = eb.act[l] = (unsigned char)on; ea.live[l] = eb.live[l] = (unsigned char)on;
                    }
                    /* (the kernel's loop body is exec-masked to `need` lanes already: V_ALL32 prices masked lanes too, which overstates it a little) */
                    priceSpan(S_EXA, &ea, 16, NULL); priceSpan(S_EXB, &eb, 16, NULL);
                    for (k = 0; k < WPW; k++) if (need[k]) {
                        U32 const fullEnd = bq[k] + bfwd[k];                     /* the oracle measured the whole length already */
                        if (pos[k] + 16u * (U32)LPW > fullEnd || pos[k] + 16u * (U32)LPW >= wk[k].limit) need[k] = 0; else { pos[k] += 16u * (U32)LPW; anyNeed = 1; }
                    }
                }
            }
        }
        for (k = 0; k < nw; k++) { stepsOf[r0 + k] = wk[k].steps; rangeSteps += wk[k].steps; rangesWalked++; }
    }
    parkUnit(stepsOf, nRanges, WPW);
}

int sim_run(const BYTE *data, size_t n, U32 unit, int level, int pad)
{
    EParams const prm = paramsForLevel(level);
    Work *w = (Work *)calloc(1, sizeof(Work));
    PAD = pad; LPW = prm.windowGroups;
    memset(cyc, 0, sizeof cyc); memset(ins, 0, sizeof ins); waveSteps = laneStepsActive = laneStepsAll = extRounds = rangeSteps = rangesWalked = 0; memset(parkSteps, 0, sizeof parkSteps);
    size_t units = 0;
    for (size_t o = 0; o + unit <= n; o += unit, units++) simUnit(w, data + o, unit, &prm);
    printf("units %zu of %u bytes, level %d, PAD %d: wave steps / unit %.1f, active lane-steps %.1f %%, extension rounds / wave step %.2f\n", units, unit, level, pad,
           (double)waveSteps / units, 100.0 * laneStepsActive / laneStepsAll, (double)extRounds / waveSteps);
    printf("walker steps / range %.1f; park the last <= T walkers of a wavefront and re-pack them, wave steps against today's:", (double)rangeSteps / rangesWalked);
    for (int t = 0; t < NPARK; t++) printf("  T=%u %.1f %%", parkT[t], 100.0 * parkSteps[t] / waveSteps);
    printf("\n");
    printf("%-22s", "LDS cycles / wave step");
    for (int s = 0; s < NSITE; s++) printf("%10s", siteName[s]);
    printf("%10s %8s\n", "total", "instr");
    for (int v = 0; v < NVAR; v++) {
        double t = 0, ti = 0;
        printf("%-22s", varName[v]);
        for (int s = 0; s < NSITE; s++) { printf("%10.1f", cyc[v][s] / waveSteps); t += cyc[v][s]; ti += ins[v][s]; }
        printf("%10.1f %8.1f\n", t / waveSteps, ti / waveSteps);
    }
    free(w);
    return 0;
}
