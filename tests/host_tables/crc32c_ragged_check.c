/*
 * CPU check of the ragged CRC32C checksum (crc_kernels.hip crc32c_shards_rag
 * and crc32c_combine_rag) on the engine's own host tables (crc_host.c,
 * included): the length-independent image isal_hip_crc32c_ragged_image is
 * built for tt = 2 and tt = 64, and for each length every lane of the pass and
 * of the combine is emulated as the kernels compute it, from that image alone:
 *   pass     b' = F'(w0 ^ b, w1, w2, w3) over the block's full tiles (last: F),
 *            the ragged tile's chunk CRCs (the straddling lane bytewise);
 *   combine  Horner over the blocks through the byte tables of x^(8*4096*tt),
 *            the last block through PW[nfull_last], W[L] and Ct[L] from X,
 *            x^(8*len) = X[r] * the wave product of SQ over the bits of nfull.
 * The result is compared with the bytewise CRC, and the derived constants with
 * isal_hip_crc32c_plan(len, tt) word for word. Test infrastructure only.
 */
#include <stdio.h>
#include <stdlib.h>

#include "../../isa-l_amd/csrc/crc_host.c"

#define T ISAL_HIP_CRC_TILE

static uint32_t
fields32(const uint32_t *t, const uint32_t w[4])
{
        uint32_t r = 0;
        int d, f;
        for (d = 0; d < 4; d++)
                for (f = 0; f < ISAL_HIP_CRC_FIELDS; f++)
                        r ^= t[(d * ISAL_HIP_CRC_FIELDS + f) * 32 +
                               ((w[d] >> field_lo(f)) & ((1u << field_bits(f)) - 1))];
        return r;
}

static uint32_t
bytewise(const uint32_t *t0tab, uint32_t c, const uint8_t *p, long long n)
{
        long long i;
        for (i = 0; i < n; i++)
                c = (c >> 8) ^ t0tab[(c ^ p[i]) & 0xff];
        return c;
}

static uint32_t
byte_tables_mul(const uint32_t *k4, uint32_t h)
{
        return k4[h & 0xff] ^ k4[256 + ((h >> 8) & 0xff)] ^ k4[512 + ((h >> 16) & 0xff)] ^ k4[768 + (h >> 24)];
}

/* lanes 0..31 of wave_product32: factor i = SQ[i] where bit i of nfull is set */
static uint32_t
wave_product(const uint32_t *im, unsigned nfull)
{
        uint32_t v[32], n[32];
        int lane, m;
        for (lane = 0; lane < 32; lane++) {
                const uint32_t sq = lane < ISAL_HIP_CRC_RAG_NSQ ? im[ISAL_HIP_CRC_RAG_SQ + lane] : 0x80000000u;
                v[lane] = (nfull >> lane) & 1u ? sq : 0x80000000u;
        }
        for (m = 16; m >= 1; m >>= 1) {
                for (lane = 0; lane < 32; lane++)
                        n[lane] = isal_hip_crc32c_mulmod(v[lane], v[lane ^ m]);
                memcpy(v, n, sizeof(v));
        }
        return v[0];
}

/* what the combine derives for a shard of len > 0 bytes */
typedef struct {
        unsigned nfull, r, nblk, nfull_last;
        uint32_t klast, xlen, w[256], ct[256];
} derived;

static void
derive(const uint32_t *im, int tt, long long len, derived *d)
{
        const uint32_t *X = im + ISAL_HIP_CRC_RAG_X;
        unsigned ntiles, done;
        int L;
        d->nfull = (unsigned) (len / T);
        d->r = (unsigned) (len % T);
        ntiles = d->nfull + (d->r ? 1 : 0);
        d->nblk = (ntiles + tt - 1) / tt;
        done = (d->nblk - 1) * tt;
        d->nfull_last = d->nfull > done ? d->nfull - done : 0;
        d->klast = im[ISAL_HIP_CRC_RAG_PW + d->nfull_last];
        for (L = 0; L < 256; L++) {
                const int rest = (int) d->r - 16 * L - 16;
                d->w[L] = X[16 * (255 - L) + d->r];
                d->ct[L] = X[rest > 0 ? rest : 0];
        }
        d->xlen = isal_hip_crc32c_mulmod(wave_product(im, d->nfull), X[d->r]);
}

static uint32_t
emulate(const uint32_t *im, int tt, const uint8_t *buf, long long len, uint32_t init)
{
        const uint32_t *F = im + ISAL_HIP_CRC_CHUNK_TAB, *FZ = im + ISAL_HIP_CRC_RAG_FPRE;
        derived d;
        uint32_t *part, tail[256], v = 0;
        unsigned blk, ntiles;
        int L;
        if (len == 0)
                return init;
        derive(im, tt, len, &d);
        ntiles = d.nfull + (d.r ? 1 : 0);
        part = calloc((size_t) d.nblk * 256, 4);
        memset(tail, 0xEE, sizeof(tail)); /* every lane of a ragged tile writes its slot */
        for (blk = 0; blk < d.nblk; blk++) { /* crc32c_shards_rag, one item */
                const unsigned t0 = blk * tt, t1 = t0 + tt < ntiles ? t0 + tt : ntiles;
                const unsigned tf = t1 < d.nfull ? t1 : d.nfull;
                for (L = 0; L < 256; L++) {
                        uint32_t b = 0, w[4];
                        unsigned t;
                        for (t = t0; t < tf; t++) {
                                memcpy(w, buf + (size_t) t * T + 16 * L, 16);
                                w[0] ^= b;
                                b = fields32(t + 1 == tf ? F : FZ, w);
                        }
                        if (tf < t1) {
                                const long long off = (long long) tf * T + 16 * L, left = len - off;
                                const int nb = left >= 16 ? 16 : (left > 0 ? (int) left : 0);
                                uint32_t c = 0;
                                if (nb == 16) {
                                        memcpy(w, buf + off, 16);
                                        c = fields32(F, w);
                                } else if (nb > 0) {
                                        c = bytewise(im, 0, buf + off, nb);
                                }
                                tail[L] = c;
                        }
                        part[(size_t) blk * 256 + L] = b;
                }
        }
        for (L = 0; L < 256; L++) { /* crc32c_combine_rag, lane position L */
                uint32_t h = 0;
                unsigned b;
                for (b = 0; b + 1 < d.nblk; b++)
                        h = byte_tables_mul(im + ISAL_HIP_CRC_RAG_BLOCK, h) ^ part[(size_t) b * 256 + L];
                h = (d.nblk > 1 ? isal_hip_crc32c_mulmod(h, d.klast) : 0) ^ part[(size_t) (d.nblk - 1) * 256 + L];
                v ^= isal_hip_crc32c_mulmod(h, d.w[L]);
                if (d.r)
                        v ^= isal_hip_crc32c_mulmod(tail[L], d.ct[L]);
        }
        free(part);
        return v ^ isal_hip_crc32c_mulmod(init, d.xlen);
}

/* the derived constants against the per-length plan of the uniform batch */
static int
plan_check(const uint32_t *im, int tt, long long len)
{
        static uint32_t plan[ISAL_HIP_CRC_PLAN_DWORDS], last[1024];
        isal_hip_crc_geom g;
        derived d;
        int bad = 0;
        derive(im, tt, len, &d);
        isal_hip_crc32c_plan(len, tt, plan);
        isal_hip_crc_geometry(len, tt, &g);
        if (g.nblk != (long long) d.nblk || g.nfull_last != (long long) d.nfull_last) {
                printf("len %lld tt %d: geometry nblk %u/%lld nfull_last %u/%lld\n", len, tt, d.nblk, g.nblk,
                       d.nfull_last, g.nfull_last);
                bad = 1;
        }
        mul_tables(d.klast, last);
        if (memcmp(im + ISAL_HIP_CRC_RAG_BLOCK, plan + ISAL_HIP_CRC_PLAN_BLOCK, 4096)) {
                printf("len %lld tt %d: block tables differ from the plan\n", len, tt);
                bad = 1;
        }
        if (memcmp(last, plan + ISAL_HIP_CRC_PLAN_LAST, 4096)) {
                printf("len %lld tt %d: last-block multiplier differs from the plan\n", len, tt);
                bad = 1;
        }
        if (memcmp(d.w, plan + ISAL_HIP_CRC_PLAN_W, 1024) || memcmp(d.ct, plan + ISAL_HIP_CRC_PLAN_CT, 1024)) {
                printf("len %lld tt %d: W or Ct differs from the plan\n", len, tt);
                bad = 1;
        }
        if (d.xlen != plan[ISAL_HIP_CRC_PLAN_XLEN]) {
                printf("len %lld tt %d: x^(8 len) %08x, plan %08x\n", len, tt, d.xlen, plan[ISAL_HIP_CRC_PLAN_XLEN]);
                bad = 1;
        }
        return bad;
}

#define GUARD_WORDS 64
#define GUARD 0xA5C3F00Du

int
main(void)
{
        static const int tts[2] = { 2, 64 };
        static const uint32_t inits[3] = { 0, 0xFFFFFFFFu, 0x1B2E3D4Cu };
        const long long maxlen = 3LL * 64 * T;
        uint8_t *buf = malloc((size_t) maxlen);
        long long i;
        int g, bad = 0, ncases = 0;
        srand(29);
        for (i = 0; i < maxlen; i++)
                buf[i] = (uint8_t) rand();
        for (g = 0; g < 2; g++) {
                const int tt = tts[g];
                const long long B = (long long) tt * T;
                const size_t n = isal_hip_crc32c_ragged_image_dwords(tt);
                uint32_t *im = malloc(4 * (n + GUARD_WORDS)), *other = malloc(4 * (n + GUARD_WORDS));
                long long lens[13 + 200];
                int nl = 0, c, j;
                const long long listed[13] = { 0, 1, 5, 16, T - 1, T, T + 1, T + 16, B, B + 1, B + T,
                                               2 * B + 3 * 16 + 7, 3 * B };
                for (j = 0; j < (int) (n + GUARD_WORDS); j++)
                        im[j] = GUARD;
                isal_hip_crc32c_ragged_image(tt, im);
                for (j = 0; j < GUARD_WORDS; j++)
                        if (im[n + j] != GUARD) {
                                printf("tt %d: guard word %d after the image overwritten\n", tt, j);
                                bad = 1;
                        }
                /* everything but the block tables and PW's length is the same for every tt */
                isal_hip_crc32c_ragged_image(tt == 2 ? 3 : 2, other);
                if (memcmp(im, other, 4 * ISAL_HIP_CRC_RAG_BLOCK) ||
                    memcmp(im + ISAL_HIP_CRC_RAG_X, other + ISAL_HIP_CRC_RAG_X,
                           4 * (ISAL_HIP_CRC_RAG_PW + 3 - ISAL_HIP_CRC_RAG_X))) {
                        printf("tt %d: a length-independent table depends on tt\n", tt);
                        bad = 1;
                }
                for (j = 0; j < ISAL_HIP_CRC_RAG_X_DWORDS; j += 257)
                        if (im[ISAL_HIP_CRC_RAG_X + j] != isal_hip_crc32c_xpow8n((unsigned long long) j)) {
                                printf("tt %d: X[%d] is not x^(8*%d)\n", tt, j, j);
                                bad = 1;
                        }
                for (j = 0; j < 13; j++)
                        lens[nl++] = listed[j];
                for (j = 0; j < 200; j++)
                        lens[nl++] = rand() % (40 * 1024);
                for (j = 0; j < nl; j++) {
                        const uint8_t *p = buf + (j % 7) * 16; /* another window of the data per case */
                        if (lens[j] + 7 * 16 > maxlen)
                                p = buf;
                        if (lens[j] > 0)
                                bad |= plan_check(im, tt, lens[j]);
                        for (c = 0; c < 3; c++) {
                                const uint32_t got = emulate(im, tt, p, lens[j], inits[c]);
                                const uint32_t want = bytewise(im, inits[c], p, lens[j]);
                                ncases++;
                                if (got != want) {
                                        printf("tt %d len %lld init %08x: emulated %08x, bytewise %08x\n", tt, lens[j],
                                               inits[c], got, want);
                                        bad = 1;
                                }
                        }
                }
                free(im);
                free(other);
        }
        free(buf);
        if (bad) {
                printf("FAIL\n");
                return 1;
        }
        printf("ragged crc32c pass and combine ok (%d cases); derived constants equal the per-length plan\n", ncases);
        return 0;
}
