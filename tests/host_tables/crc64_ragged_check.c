/*
 * CPU check of the ragged CRC64 checksum (crc64_kernels.hip crc64_shards_rag
 * and crc64_combine_rag) on the engine's own host tables (crc64_host.c,
 * included), for all eight flavours:
 *   ring     isal_hip_crc64_mulmod / isal_hip_crc64_xpow8n against the matrix
 *            form Z^n (isal_hip_crc64_zpow) on 1000 seeded values and exponents;
 *   image    isal_hip_crc64_ragged_image for tt = 2 and tt = 128 (the default);
 *   kernels  for each length every lane of the pass and of the combine is
 *            emulated as the kernels compute it, from that image alone:
 *              pass     b' = F'_u(chunk ^ b) over the block's full tiles (last:
 *                       F_u), two dwords of b into the chunk's first 8 bytes;
 *              combine  Horner over all but the last block through the field
 *                       tables of Z^(4096*tt) (V), the last block's chains (P)
 *                       and the tail's chunks, right-aligned (T), each through
 *                       wave_fold lane by lane; then the one product phase:
 *                       lanes 0..31 multiply SQ over the bits of nfull,
 *                       X[len % 4096] and ~init, lanes 32..39 V, PW[nfull_last]
 *                       and X[16q], lanes 40..47 P and X[16q], with the 64-step
 *                       shift-and-XOR product as the device runs it; the last
 *                       bytes through the byte table;
 *            and compared with a bytewise CRC built from raw_update alone;
 *   plan     what the combine derives for a length against the maps
 *            isal_hip_crc64_len_tables tabulates for it (OP_BLOCK, OP_LAST,
 *            OP_TAIL) and against isal_hip_crc64_init_term, each applied to the
 *            64 basis values.
 * Test infrastructure only.
 */
#include <stdio.h>
#include <stdlib.h>

#include "../../isa-l_amd/csrc/crc64_host.c"

#define T ISAL_HIP_CRC_TILE
#define NV NFLAVOURS

static uint64_t seed_state = 0x9E3779B97F4A7C15ULL;

static uint64_t
rnd64(void)
{
        /* xorshift64* */
        seed_state ^= seed_state >> 12;
        seed_state ^= seed_state << 25;
        seed_state ^= seed_state >> 27;
        return seed_state * 0x2545F4914F6CDD1DULL;
}

/* the reference's byte loop on a table built bit by bit: the checker */
static uint64_t ref_tab[NV][256];

static uint64_t
bytewise(int variant, uint64_t init, const uint8_t *p, long long n)
{
        const int refl = isal_hip_crc64_is_refl(variant);
        uint64_t s = ~init;
        long long i;
        for (i = 0; i < n; i++)
                s = refl ? ref_tab[variant][(s ^ p[i]) & 0xff] ^ (s >> 8)
                         : ref_tab[variant][((s >> 56) ^ p[i]) & 0xff] ^ (s << 8);
        return ~s;
}

/* the device's crc64_mulmod<REFL>: 64 branch-free steps on register pairs, the
 * coefficient's mask extracted from a's dword without shifting a */
static uint64_t
dev_mulmod(int refl, uint64_t a, uint64_t b, uint64_t poly)
{
        const uint32_t ql = (uint32_t) poly, qh = (uint32_t) (poly >> 32);
        uint32_t bl = (uint32_t) b, bh = (uint32_t) (b >> 32), pl = 0, ph = 0;
        int half, i;
        for (half = 0; half < 2; half++) {
                const uint32_t w = (uint32_t) ((half == 0) == (refl != 0) ? a >> 32 : a);
                for (i = 0; i < 32; i++) {
                        const uint32_t ma = 0u - ((w >> (refl ? 31 - i : i)) & 1u);
                        uint32_t mb;
                        pl ^= bl & ma;
                        ph ^= bh & ma;
                        if (refl) {
                                mb = 0u - (bl & 1u);
                                bl = (bl >> 1) | (bh << 31);
                                bh >>= 1;
                        } else {
                                mb = 0u - (bh >> 31);
                                bh = (bh << 1) | (bl >> 31);
                                bl <<= 1;
                        }
                        bl ^= ql & mb;
                        bh ^= qh & mb;
                }
        }
        return (uint64_t) ph << 32 | pl;
}

/* a map stored as 14 field tables (crc_device.h lookup14 / apply_op) */
static uint64_t
fields_op(const uint64_t *t, uint64_t v)
{
        uint64_t r = 0;
        int h, f;
        for (h = 0; h < 2; h++)
                for (f = 0; f < ISAL_HIP_CRC_FIELDS; f++)
                        r ^= t[(h * ISAL_HIP_CRC_FIELDS + f) * 32 +
                               (((uint32_t) (v >> (32 * h)) >> field_lo(f)) & field_mask(f))];
        return r;
}

/* a chunk map stored as 28 field tables (crc_device.h chunk_acc) */
static uint64_t
fields_chunk(const uint64_t *t, const uint32_t w[4])
{
        uint64_t r = 0;
        int d, f;
        for (d = 0; d < 4; d++)
                for (f = 0; f < ISAL_HIP_CRC_FIELDS; f++)
                        r ^= t[(d * ISAL_HIP_CRC_FIELDS + f) * 32 + ((w[d] >> field_lo(f)) & field_mask(f))];
        return r;
}

/* wave_fold: lane l holds positions 4l..4l+3; lanes past the wave are garbage */
static uint64_t
wave_fold(const uint64_t *tree, const uint64_t pos[256])
{
        uint64_t h[64 + 32], n[64];
        int l, i, s;
        for (l = 0; l < 64; l++) {
                h[l] = pos[4 * l];
                for (i = 1; i < 4; i++)
                        h[l] = fields_op(tree, h[l]) ^ pos[4 * l + i];
        }
        for (s = 0; s < 6; s++) {
                for (l = 64; l < 96; l++)
                        h[l] = 0xBADBADBADBADBADBULL ^ (uint64_t) l; /* what a shuffle past the wave may return */
                for (l = 0; l < 64; l++)
                        n[l] = fields_op(tree + (s + 2) * ISAL_HIP_CRC64_OP_ENTRIES, h[l]) ^ h[l + (1 << s)];
                memcpy(h, n, sizeof(n));
        }
        return h[0];
}

/* what the combine derives for a shard of len > 0 bytes */
typedef struct {
        unsigned nfull, tail, q, rem, nblk, nfull_last;
        uint64_t klast, ktail;
} derived;

static void
derive(const uint64_t *im, int tt, long long len, derived *d)
{
        unsigned ntiles, done;
        d->nfull = (unsigned) (len / T);
        d->tail = (unsigned) (len % T);
        d->q = d->tail / 16;
        d->rem = d->tail % 16;
        ntiles = d->nfull + (d->tail ? 1 : 0);
        d->nblk = (ntiles + tt - 1) / tt;
        done = (d->nblk - 1) * tt;
        d->nfull_last = d->nfull > done ? d->nfull - done : 0;
        d->klast = im[ISAL_HIP_CRC64_RAG_PW + d->nfull_last];
        d->ktail = im[ISAL_HIP_CRC64_RAG_X + 16 * d->q];
}

/* The combine's factors lane by lane and wave_products64: lanes 0..31 one
 * product (SQ[i] where bit i of nfull is set, X[len % 4096], ~init), lanes
 * 32..39 V * PW[nfull_last] * X[16q], lanes 40..47 P * X[16q]; the upper half
 * skips the steps across its groups of eight. */
static void
wave_products(int variant, const uint64_t *im, const derived *d, uint64_t init, uint64_t xv, uint64_t xp,
              uint64_t f[64])
{
        const int refl = isal_hip_crc64_is_refl(variant);
        const uint64_t poly = isal_hip_crc64_ring_poly(variant), one = refl ? 1ULL << 63 : 1ULL;
        uint64_t n[64];
        int lane, m;
        for (lane = 0; lane < 64; lane++)
                f[lane] = one;
        for (lane = 0; lane < ISAL_HIP_CRC64_RAG_NSQ; lane++)
                if ((d->nfull >> lane) & 1u)
                        f[lane] = im[ISAL_HIP_CRC64_RAG_SQ + lane];
        f[ISAL_HIP_CRC64_RAG_NSQ] = im[ISAL_HIP_CRC64_RAG_X + d->tail];
        f[ISAL_HIP_CRC64_RAG_NSQ + 1] = ~init;
        f[32] = xv;
        f[33] = d->klast;
        f[34] = d->ktail;
        f[40] = xp;
        f[41] = d->ktail;
        for (m = 1; m <= 16; m <<= 1) {
                for (lane = 0; lane < 64; lane++)
                        n[lane] = m < 8 || lane < 32 ? dev_mulmod(refl, f[lane], f[lane ^ m], poly) : f[lane];
                memcpy(f, n, sizeof(n));
        }
}

static uint64_t
emulate(int variant, const uint64_t *im, int tt, const uint8_t *buf, long long len, uint64_t init)
{
        const int refl = isal_hip_crc64_is_refl(variant);
        const uint64_t *Fu = im + ISAL_HIP_CRC64_RAG_PRE, *FZu = Fu + ISAL_HIP_CRC64_CHUNK_ENTRIES;
        const uint64_t *tree = im + ISAL_HIP_CRC64_RAG_TREE;
        derived d;
        uint64_t *part, pos[256], f[64], xv = 0, xp = 0, tq = 0, s;
        unsigned blk, j;
        int L;
        if (len == 0)
                return init;
        derive(im, tt, len, &d);
        part = malloc((size_t) d.nblk * 256 * 8);
        memset(part, 0xEE, (size_t) d.nblk * 256 * 8); /* every lane of every item writes its slot */
        for (blk = 0; blk < d.nblk; blk++) {           /* crc64_shards_rag, one item */
                const unsigned t0 = blk * tt, t1 = t0 + tt < d.nfull ? t0 + tt : d.nfull;
                for (L = 0; L < 256; L++) {
                        uint64_t b = 0;
                        uint32_t w[4];
                        unsigned t;
                        for (t = t0; t < t1; t++) {
                                memcpy(w, buf + (size_t) t * T + 16 * L, 16);
                                w[0] ^= (uint32_t) b;
                                w[1] ^= (uint32_t) (b >> 32);
                                b = fields_chunk(t + 1 == t1 ? Fu : FZu, w);
                        }
                        part[(size_t) blk * 256 + L] = refl ? b : __builtin_bswap64(b);
                }
        }
        if (d.nfull) { /* crc64_combine_rag */
                if (d.nblk > 1) {
                        for (L = 0; L < 256; L++) {
                                uint64_t v = 0;
                                for (blk = 0; blk + 1 < d.nblk; blk++)
                                        v = fields_op(im + ISAL_HIP_CRC64_RAG_BLOCK, v) ^ part[(size_t) blk * 256 + L];
                                pos[L] = v;
                        }
                        xv = wave_fold(tree, pos);
                }
                xp = wave_fold(tree, part + (size_t) (d.nblk - 1) * 256);
        }
        if (d.q) {
                for (L = 0; L < 256; L++) {
                        const int c = L - (256 - (int) d.q);
                        uint32_t w[4];
                        pos[L] = 0;
                        if (c >= 0) {
                                memcpy(w, buf + (size_t) d.nfull * T + (size_t) c * 16, 16);
                                pos[L] = fields_chunk(im + ISAL_HIP_CRC64_RAG_CHUNK, w);
                        }
                }
                tq = wave_fold(tree, pos);
        }
        wave_products(variant, im, &d, init, xv, xp, f);
        s = f[32] ^ f[40] ^ tq;
        for (j = 0; j < d.rem; j++) {
                const uint8_t byte = buf[len - d.rem + j];
                s = refl ? im[ISAL_HIP_CRC64_RAG_BYTE + ((s ^ byte) & 0xff)] ^ (s >> 8)
                         : im[ISAL_HIP_CRC64_RAG_BYTE + (((s >> 56) ^ byte) & 0xff)] ^ (s << 8);
        }
        free(part);
        return ~(f[0] ^ s);
}

/* the derived constants against the per-length maps of the uniform batch */
static int
plan_check(int variant, const uint64_t *im, int tt, long long len)
{
        static uint64_t tabs[ISAL_HIP_CRC64_TAB_ENTRIES];
        const int refl = isal_hip_crc64_is_refl(variant);
        const uint64_t poly = isal_hip_crc64_ring_poly(variant);
        isal_hip_crc64_geom g;
        derived d;
        uint64_t f[64];
        int bad = 0, i;
        derive(im, tt, len, &d);
        isal_hip_crc64_geometry(len, tt, &g);
        isal_hip_crc64_len_tables(variant, len, tt, tabs);
        if (g.nfull != (long long) d.nfull || g.tail != (int) d.tail) {
                printf("v %d len %lld tt %d: nfull %u/%lld tail %u/%d\n", variant, len, tt, d.nfull, g.nfull, d.tail, g.tail);
                bad = 1;
        }
        /* The uniform geometry counts blocks of full tiles only; the item table
         * counts the ragged tile too, so a tail behind a whole number of full
         * blocks is a last block without a full tile: Z^0 after one more Z^(4096*tt). */
        if ((long long) d.nblk == g.nblk ? (long long) d.nfull_last != g.nfull_last
                                         : !((long long) d.nblk == g.nblk + 1 && d.nfull_last == 0 && d.tail &&
                                             (g.nblk == 0 || g.nfull_last == g.tt))) {
                printf("v %d len %lld tt %d: geometry nblk %u/%lld nfull_last %u/%lld\n", variant, len, tt, d.nblk,
                       g.nblk, d.nfull_last, g.nfull_last);
                bad = 1;
        }
        if (memcmp(im + ISAL_HIP_CRC64_RAG_BLOCK, tabs + ISAL_HIP_CRC64_OP_BLOCK, ISAL_HIP_CRC64_OP_ENTRIES * 8)) {
                printf("v %d len %lld tt %d: block tables differ from the plan\n", variant, len, tt);
                bad = 1;
        }
        for (i = 0; i < 64; i++) {
                const uint64_t e = 1ULL << i;
                const uint64_t last = (long long) d.nblk == g.nblk
                                              ? dev_mulmod(refl, e, d.klast, poly)
                                              : fields_op(im + ISAL_HIP_CRC64_RAG_BLOCK, dev_mulmod(refl, e, d.klast, poly));
                if (g.nblk && last != fields_op(tabs + ISAL_HIP_CRC64_OP_LAST, e)) {
                        printf("v %d len %lld tt %d: last-block multiplier differs from OP_LAST on bit %d\n", variant,
                               len, tt, i);
                        bad = 1;
                }
                if (dev_mulmod(refl, e, d.ktail, poly) != fields_op(tabs + ISAL_HIP_CRC64_OP_TAIL, e)) {
                        printf("v %d len %lld tt %d: X[16q] differs from OP_TAIL on bit %d\n", variant, len, tt, i);
                        bad = 1;
                }
                wave_products(variant, im, &d, e, 0, 0, f);
                if (f[0] != isal_hip_crc64_init_term(variant, len, e)) {
                        printf("v %d len %lld tt %d: x^(8 len) differs from the init term on bit %d\n", variant, len,
                               tt, i);
                        bad = 1;
                }
        }
        return bad;
}

static int
ring_check(int variant)
{
        const int refl = isal_hip_crc64_is_refl(variant);
        const uint64_t poly = isal_hip_crc64_ring_poly(variant), one = refl ? 1ULL << 63 : 1ULL;
        uint64_t m[64];
        int i, bad = 0;
        for (i = 0; i < 1000 && !bad; i++) {
                /* exponents of every size: up to 2^(i % 40) bytes */
                const unsigned long long n = rnd64() & ((2ULL << (i % 40)) - 1);
                const uint64_t v = i < 64 ? 1ULL << i : rnd64(), xn = isal_hip_crc64_xpow8n(variant, n);
                isal_hip_crc64_zpow(variant, n, m);
                if (isal_hip_crc64_mulmod(variant, v, xn) != apply(m, v) || isal_hip_crc64_mulmod(variant, xn, v) != apply(m, v) ||
                    dev_mulmod(refl, v, xn, poly) != apply(m, v) || xn != apply(m, one)) {
                        printf("v %d: x^(8*%llu) * %016llx differs from Z^n\n", variant, n, (unsigned long long) v);
                        bad = 1;
                }
        }
        return bad;
}

#define GUARD_WORDS 64
#define GUARD 0xA5C3F00DA5C3F00DULL
#define NLISTED 15
#define NRANDOM 200

int
main(void)
{
        static const int tts[2] = { 2, 128 };
        const uint64_t inits[3] = { 0, ~0ULL, 0x1B2E3D4C5A697887ULL };
        const long long maxlen = 3LL * 128 * T + 7 * 16;
        uint8_t *buf = malloc((size_t) maxlen);
        long long i;
        int variant, g, bad = 0, ncases = 0;
        for (i = 0; i < maxlen; i++)
                buf[i] = (uint8_t) (rnd64() >> 56);
        for (variant = 0; variant < NV; variant++) {
                const int refl = isal_hip_crc64_is_refl(variant);
                for (i = 0; i < 256; i++)
                        ref_tab[variant][i] = raw_update(variant, refl ? (uint64_t) i : (uint64_t) i << 56, NULL, 1);
                bad |= ring_check(variant);
                for (g = 0; g < 2; g++) {
                        const int tt = tts[g];
                        const long long B = (long long) tt * T;
                        const size_t n = isal_hip_crc64_ragged_image_entries(tt);
                        uint64_t *im = malloc(8 * (n + GUARD_WORDS)), *other = malloc(8 * (n + GUARD_WORDS));
                        long long lens[NLISTED + NRANDOM];
                        int nl = 0, c, j;
                        const long long listed[NLISTED] = { 0, 1, 5, 15, 16, 17, T - 1, T, T + 1, T + 16, B, B + 1, B + T,
                                                            2 * B + 55, 3 * B };
                        for (j = 0; j < (int) (n + GUARD_WORDS); j++)
                                im[j] = GUARD;
                        isal_hip_crc64_ragged_image(variant, tt, im);
                        for (j = 0; j < GUARD_WORDS; j++)
                                if (im[n + j] != GUARD) {
                                        printf("v %d tt %d: guard word %d after the image overwritten\n", variant, tt, j);
                                        bad = 1;
                                }
                        /* everything but the block tables and PW's length is the same for every tt */
                        isal_hip_crc64_ragged_image(variant, tt == 2 ? 3 : 2, other);
                        if (memcmp(im, other, 8 * ISAL_HIP_CRC64_RAG_BLOCK) ||
                            memcmp(im + ISAL_HIP_CRC64_RAG_TREE, other + ISAL_HIP_CRC64_RAG_TREE,
                                   8 * (ISAL_HIP_CRC64_RAG_PW + 3 - ISAL_HIP_CRC64_RAG_TREE))) {
                                printf("v %d tt %d: a length-independent table depends on tt\n", variant, tt);
                                bad = 1;
                        }
                        for (j = 0; j < ISAL_HIP_CRC64_RAG_X_ENTRIES; j += 257)
                                if (im[ISAL_HIP_CRC64_RAG_X + j] != isal_hip_crc64_xpow8n(variant, (unsigned long long) j)) {
                                        printf("v %d tt %d: X[%d] is not x^(8*%d)\n", variant, tt, j, j);
                                        bad = 1;
                                }
                        for (j = 0; j < NLISTED; j++)
                                lens[nl++] = listed[j];
                        for (j = 0; j < NRANDOM; j++)
                                lens[nl++] = (long long) (rnd64() % (40 * 1024));
                        for (j = 0; j < nl; j++) {
                                const uint8_t *p = buf + (j % 7) * 16; /* another window of the data per case */
                                if (lens[j] > 0)
                                        bad |= plan_check(variant, im, tt, lens[j]);
                                for (c = 0; c < 3; c++) {
                                        const uint64_t got = emulate(variant, im, tt, p, lens[j], inits[c]);
                                        const uint64_t want = bytewise(variant, inits[c], p, lens[j]);
                                        ncases++;
                                        if (got != want) {
                                                printf("v %d tt %d len %lld init %016llx: emulated %016llx, bytewise %016llx\n",
                                                       variant, tt, lens[j], (unsigned long long) inits[c],
                                                       (unsigned long long) got, (unsigned long long) want);
                                                bad = 1;
                                        }
                                }
                        }
                        free(im);
                        free(other);
                }
        }
        free(buf);
        if (bad) {
                printf("FAIL\n");
                return 1;
        }
        printf("ragged crc64 ring, pass and combine ok (%d cases, 8 variants); derived constants equal the per-length maps\n",
               ncases);
        return 0;
}
