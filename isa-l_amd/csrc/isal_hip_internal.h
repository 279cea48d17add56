/*
 * isal_hip_internal.h — contract between the C host code (the drop-in shim:
 * isal_hip_shim.c and the units listed in isal_hip_shim.h; the batch API in
 * isal_hip_batch.c; gf_host.c) and the HIP kernel launchers (ec_kernels.hip).
 * Not installed.
 *
 * Device argument layout (one contiguous device allocation per call or batch):
 *
 *   ptrs : uint64_t[nstripes][ptr_stride]   shard device addresses; for a
 *          stripe s, sources at [s][src_idx0 + j], outputs at [s][dst_idx0 + l]
 *   tbl  : uint32_t coefficient tables, grouped by row pass g (rows r0..r0+P-1,
 *          P <= EC_MAX_ROWS_PER_PASS): group g starts at dword 5*k*r0 and is
 *          laid out [j < k][l < P][5], so one source's tables for every output
 *          of the pass are contiguous (one scalar-load burst per source).
 *
 * The 5 dwords of one coefficient c are three v_perm_b32 byte-lookup tables
 * (GF(2^8) multiplication is GF(2)-linear, so c*x = c*(x&7) ^ c*(x&0x38) ^ c*(x&0xc0)):
 *   [0],[1]  c*{0,1,..,7}             (entries 0-3 in [0], 4-7 in [1])
 *   [2],[3]  c*{0,8,16,..,56}
 *   [4]      c*{0,64,128,192}
 */
#ifndef ISAL_HIP_INTERNAL_H
#define ISAL_HIP_INTERNAL_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EC_MAX_ROWS_PER_PASS 8
#define EC_TBL_DWORDS 5

/* Host GF math (gf_host.c). */
unsigned char isal_hip_gf_mul(unsigned char a, unsigned char b);
/* Fill the grouped perm tables above from 32-byte-per-coefficient gftbls
 * (only byte 1 of each 32 B entry, the coefficient itself, is read — exactly
 * what ec_base.c reads, so any gftbls gives the reference's answer). */
void isal_hip_build_tables(int k, int rows, const unsigned char *gftbls, uint32_t *tbl);
size_t isal_hip_tables_dwords(int k, int rows);

/* 0/1 structure of an encode's coefficient passes. Every gf_gen_rs_matrix
 * parity block has row 0 = all ones and column 0 = all ones (ec_base.c
 * gf_gen_rs_matrix: p = 1 for j = 0, gen = 1 for the first parity row); so
 * does RAID pq_gen's. A product with a 0/1 coefficient is x & mask (one VALU
 * op per dword, or none when it starts the sum) instead of three v_perm
 * lookups and their folds. Pass g (rows 8g..8g+P-1) qualifies — bit g of
 * `ok` — when its first row and its column of source 0 hold only 0 and 1 and
 * k <= 64; then r0[g] has bit j set where row 8g's coefficient of source j is
 * 1, and c0[g] bit l where row 8g + l's coefficient of source 0 is 1.
 * The masks are computed whatever the knobs say; ISAL_HIP_ENC_XOR=0 makes the
 * launch ignore them (every pass takes the lookup path). */
#define EC_MAX_PASSES 32
typedef struct {
        unsigned ok;
        unsigned c0[EC_MAX_PASSES];
        unsigned long long r0[EC_MAX_PASSES];
        /* device copy of isal_hip_build_ldsx_tables' output, or NULL: the
         * wide passes may then look their products up in LDS (ec_kernels.hip
         * ec_encode_ldsx). isal_hip_enc_masks leaves it NULL; a caller that
         * uploads the tables sets it. */
        const uint64_t *ldsx;
} isal_hip_encmask;
void isal_hip_enc_masks(int k, int rows, const unsigned char *gftbls, isal_hip_encmask *m);

/* LDS product tables of a pass of P <= 8 rows: for each source j, a 32-entry
 * table T5_j[v] (8 bytes, byte l = c[r0 + l][j] * v: bits 0-4 of a source
 * byte) and an 8-entry table T3_j[v] (byte l = c[r0 + l][j] * (v << 5): bits
 * 5-7); pass g occupies k * ISAL_HIP_LDSX_ENTRIES words: [k][32] T5, then
 * [k][8] T3. A source byte's products with all P coefficients are two
 * lookups (T5 ^ T3). */
#define ISAL_HIP_LDSX_ENTRIES 40
size_t isal_hip_ldsx_words(int k, int rows);
void isal_hip_build_ldsx_tables(int k, int rows, const unsigned char *gftbls, uint64_t *out);
void isal_hip_build_ldsx_tables_coef(int k, int rows, const unsigned char *coef, uint64_t *out);

/* Kernel launchers (ec_kernels.hip). Return 0 or a hipError_t value.
 * `stream` is a hipStream_t. `vec16` = every shard address is 16-byte aligned. */
int isal_hip_launch_encode(const uint64_t *d_ptrs, int ptr_stride, int src_idx0, int dst_idx0,
                           const uint32_t *d_tbl, int len, int k, int rows, long long nstripes,
                           int vec16, const isal_hip_encmask *em, void *stream);
/* One stripe of device-resident, 16-byte aligned shards whose pointer table
 * (k sources then rows outputs) and coefficient tables (one pass: rows <=
 * EC_MAX_ROWS_PER_PASS, the layout above) travel as 2 KiB of kernel
 * arguments — no argument upload before the launch. Needs k + rows <=
 * ISAL_HIP_KARG_PTRS and 5 * k * rows <= ISAL_HIP_KARG_TBL. */
#define ISAL_HIP_KARG_PTRS 32
#define ISAL_HIP_KARG_TBL 448
typedef struct {
        uint64_t ptrs[ISAL_HIP_KARG_PTRS];
        uint32_t tbl[ISAL_HIP_KARG_TBL];
} isal_hip_karg;
/* Completion of a kernel-argument call without the runtime's wake-up: every
 * workgroup waits for its (write-through) stores and counts itself in *cnt;
 * the last one resets *cnt (and *res) for the next call and writes mail[1] =
 * the verify result (*res, ~0 for encode / update), then mail[0] = seq
 * (system-scope stores) into page-locked host memory that the calling thread
 * spins on (isal_hip_karg.c wait_done; ec_kernels.hip karg_done). cnt = NULL:
 * no protocol (the caller synchronises the stream). res: device word a
 * verify's mismatching lanes atomically lower (~0 between calls); NULL for
 * encode / update. */
typedef struct {
        unsigned *cnt;
        unsigned long long *res;
        unsigned long long *mail; /* device view of the host mailbox */
        unsigned long long seq;
} isal_hip_kdone;
/* cnt: ISAL_HIP_KDONE_GROUPS group counters ISAL_HIP_KDONE_STRIDE words apart
 * (one 64-byte line each), then the top counter: workgroups count in groups
 * of max(32, ceil(n / GROUPS)) and each group's last one counts in the top
 * counter — at most 256 atomics on any one word instead of one per workgroup
 * (a single word serialised 1024 workgroups' atomics: +10 us per call). */
#define ISAL_HIP_KDONE_GROUPS 256
#define ISAL_HIP_KDONE_STRIDE 16
#define ISAL_HIP_KDONE_WORDS ((ISAL_HIP_KDONE_GROUPS + 1) * ISAL_HIP_KDONE_STRIDE)
/* busy: kernel-argument calls of this process in flight, this one included
 * (chooses the lane width, ec_kernels.hip karg_narrow). */
int isal_hip_launch_encode_karg(const isal_hip_karg *a, const isal_hip_kdone *d, int len, int k, int rows,
                                const isal_hip_encmask *em, int busy, const uint64_t *ldsx, void *stream);
/* whether a drop-in encode of this shape runs on LDS product tables (then the
 * caller passes them to isal_hip_launch_encode_karg; NULL keeps v_perm) */
int isal_hip_karg_ldsx(int k, int rows);
/* ec_encode_data_update of one stripe the same way: ptrs = {source, rows
 * parity}, tbl = the source's tables for rows <= EC_MAX_ROWS_PER_PASS outputs. */
int isal_hip_launch_update_karg(const isal_hip_karg *a, const isal_hip_kdone *d, int len, int rows,
                                void *stream);
/* Verify of one stripe the same way (ptrs = k sources then rows stored
 * outputs, tables as for the encode): the first mismatch, key (column << 8 |
 * row), arrives in mail[1] (~0: none). Needs d->cnt, d->res and d->mail. */
int isal_hip_launch_verify_karg(const isal_hip_karg *a, const isal_hip_kdone *d, int len, int k, int rows,
                                const isal_hip_encmask *em, void *stream);
int isal_hip_launch_update(const uint64_t *d_ptrs, int ptr_stride, int src_idx, int dst_idx0,
                           const uint32_t *d_tbl, int len, int k, int rows, int vec_i,
                           long long nstripes, int vec16, void *stream);

/* Verify one stripe (nstripes = 1): recompute rows outputs from the sources and
 * compare with the bytes at the output pointers. Each workgroup writes the
 * minimum key (col0 + column) << 8 | row of its mismatches (~0 if none) to
 * its own slot; *nslots receives the number of slots written (at most
 * EC_VERIFY_SLOTS(rows)); the caller takes the minimum. */
#define EC_VERIFY_MAX_GRID 2048
#define EC_VERIFY_SLOTS(rows) \
        ((((rows) + EC_MAX_ROWS_PER_PASS - 1) / EC_MAX_ROWS_PER_PASS) * EC_VERIFY_MAX_GRID)
int isal_hip_launch_verify(const uint64_t *d_ptrs, int ptr_stride, int src_idx0, int dst_idx0,
                           const uint32_t *d_tbl, int len, int k, int rows, long long col0,
                           unsigned long long *slots, int *nslots, int vec16, const isal_hip_encmask *em,
                           void *stream);

/* Verify every stripe of a batch (16-byte aligned shards): bad[s] = ~0 when
 * stripe s's stored rows equal its recomputed parity, else its first
 * mismatch as column << 8 | row (bad: device memory, nstripes words, set on
 * the stream before the kernels). */
int isal_hip_launch_verify_batch(const uint64_t *d_ptrs, int ptr_stride, int src_idx0, int dst_idx0,
                                 const uint32_t *d_tbl, int len, int k, int rows, long long nstripes,
                                 const isal_hip_encmask *em, unsigned long long *bad, void *stream);

/* The shim's generic synchronous call (host or device shard pointers); fn
 * names the entry point in abort messages. op: ISAL_HIP_OP_ENCODE (dst = coded sources, nsrc = k), ISAL_HIP_OP_UPDATE
 * (dst ^= c[.][vec_i] * src[0], nsrc = 1), ISAL_HIP_OP_VERIFY (compare dst
 * with the coded sources). Returns ~0, or for VERIFY the first mismatch as
 * column << 8 | row. */
#define ISAL_HIP_OP_ENCODE 0
#define ISAL_HIP_OP_UPDATE 1
#define ISAL_HIP_OP_VERIFY 2
unsigned long long isal_hip_run(const char *fn, int op, int len, int k, int rows, int vec_i,
                                const unsigned char *gftbls, unsigned char *const *src, int nsrc,
                                unsigned char *const *dst);

/* Parity rows of a pass whose coefficients are all 0 or 1 (RS Vandermonde row
 * 0, RAID P): such a row is the XOR of some sources, so — CRC being
 * GF(2)-linear in the data — its raw CRC chains are the XOR of those sources'
 * chains. The fused encode+CRC kernels do not checksum row 0 when it is such
 * a row (bit 0 of rows; a compile-time kernel variant): they form its chains
 * from the source chains once per block. rows: bit l set for such a row l <
 * EC_MAX_ROWS_PER_PASS (k <= 64); src[l]: bit j set where c[l][j] == 1. */
typedef struct {
        unsigned rows;
        unsigned long long src[EC_MAX_ROWS_PER_PASS];
} isal_hip_xrows;
void isal_hip_xor_rows(int k, int rows, const unsigned char *gftbls, isal_hip_xrows *x);

/* Device allocations already seen by one call: a shard inside one of them is
 * device memory too, with no HIP query (a stripe's shards usually come from
 * one or two allocations: 14 queries of ~0.4 us become one or two). Only
 * within one call — a later call may find the memory freed and reused. */
#define SEEN_MAX 4
typedef struct {
        int n;
        uintptr_t lo[SEEN_MAX], hi[SEEN_MAX];
        int dev[SEEN_MAX];
} seen_t;

/* the device of the seen allocation holding [p, p + len), or -1 */
static inline int
seen_dev(const seen_t *sn, const void *p, size_t len)
{
        const uintptr_t a = (uintptr_t) p;
        int i;
        for (i = 0; i < sn->n; i++)
                if (a >= sn->lo[i] && a < sn->hi[i] && len <= sn->hi[i] - a)
                        return sn->dev[i];
        return -1;
}

static inline void
seen_add(seen_t *sn, uintptr_t base, size_t size, int dev)
{
        if (size && dev >= 0 && sn->n < SEEN_MAX) {
                sn->lo[sn->n] = base;
                sn->hi[sn->n] = base + size;
                sn->dev[sn->n] = dev;
                sn->n++;
        }
}

/* Make dev the calling thread's current device for a call on an object that
 * belongs to it; returns what isal_hip_dev_leave restores (-1: nothing, -2:
 * the switch failed). */
int isal_hip_dev_enter(int dev);
void isal_hip_dev_leave(int prev);

/* Body of an entry point on an object b that belongs to b->device (a batch,
 * a repair batch): run call there, whatever the thread's current device. */
#define ON_BATCH_DEVICE(b, call)                                                                   \
        do {                                                                                       \
                int prev_, r_;                                                                     \
                if (!(b))                                                                          \
                        return ISAL_HIP_EINVAL;                                                    \
                if ((prev_ = isal_hip_dev_enter((b)->device)) == -2)                               \
                        return ISAL_HIP_EHIP;                                                      \
                r_ = (call);                                                                       \
                isal_hip_dev_leave(prev_);                                                         \
                return r_;                                                                         \
        } while (0)

/* Every one of the n shards [ptrs[i], ptrs[i] + len) reachable by a kernel on
 * device dev: hipMalloc memory of dev, managed memory, or page-locked host
 * memory mapped at its host address (isal_hip_batch.c). ISAL_HIP_OK,
 * ISAL_HIP_EINVAL (NULL, pageable) or ISAL_HIP_EDEVICE (another GPU's). */
int isal_hip_batch_check_ptrs(const uint64_t *ptrs, size_t n, size_t len, int dev);

/* ---- what every stripe object's create does (isal_hip_objects.c): the
 * repair, overwrite, scrub and ragged batches ------------------------------ */
#define MAX_SHARDS 256 /* shard indices are bytes */
/* The n shard pointers p[] as a row of a pointer table (row may be NULL: the
 * check alone). ISAL_HIP_EINVAL unless every one is set and 16-byte aligned;
 * the whole row is written either way. */
int isal_hip_obj_ptr_row(uint64_t *row, unsigned char *const *p, size_t n);
/* isal_hip_batch_check_ptrs over a table of nrows rows of `stride` pointers:
 * the whole table at once over len bytes (lens == NULL; nothing when len ==
 * 0), or row by row over lens[row] bytes, rows of length 0 skipped. */
int isal_hip_obj_reach(const uint64_t *ptrs, size_t nrows, size_t stride, size_t len, const int *lens, int dev);
/* *d = a fresh device allocation of bytes + pad holding the bytes at h.
 * ISAL_HIP_ENOMEM when the allocation fails, ISAL_HIP_EHIP when the copy does
 * (*d is then still set: the object's destroy drops it). */
int isal_hip_obj_put(void *d, const void *h, size_t bytes, size_t pad);
/* hipFree(d) unless d is NULL */
void isal_hip_obj_drop(void *d);
/* *d = the device copy of the nitems rows isal_hip_ragged_items builds for
 * these lengths and this tile size; nothing when nitems == 0. */
int isal_hip_obj_put_items(unsigned **d, int nstripes, const int *lens, int tile, unsigned nitems);

/* Repair (ec_kernels.hip ec_repair_v16): the vector encode over nrows rows of
 * a pointer table (k survivors then rows destinations, stride ptr_stride,
 * every shard 16-byte aligned) where row r takes the coefficient tables of
 * pattern d_pat[r]: d_tbl + d_pat[r] * tbl_stride dwords, each pattern laid
 * out like one encode's tables (passes of EC_MAX_ROWS_PER_PASS rows). */
int isal_hip_launch_repair(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_pat,
                           const uint32_t *d_tbl, unsigned tbl_stride, int len, int k, int rows,
                           long long nrows, void *stream);

/* Overwrite (ec_kernels.hip ec_overwrite_v16): for each of the nstripes rows
 * of a pointer table (nw old shards, the nw new ones, then rows parity rows,
 * stride ptr_stride = 2 * nw + rows, every pointer 16-byte aligned),
 * coding[l] ^= c[l][j] * (old ^ new) with j = d_idx[row * nw + slot]; d_tbl is
 * one encode's tables (passes of EC_MAX_ROWS_PER_PASS rows). commit: the last
 * pass also stores new over old. */
int isal_hip_launch_overwrite(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_idx,
                              const uint32_t *d_tbl, int len, int k, int rows, int nw,
                              long long nstripes, int commit, void *stream);

/* Scrub (ec_kernels.hip ec_locate_v16): the batch verify (k sources then rows
 * stored rows per pointer row, every pointer 16-byte aligned, one pass:
 * 2 <= rows <= EC_MAX_ROWS_PER_PASS) whose mismatching byte columns name the
 * shard that explains their syndrome; verdict (device, nstripes words) is set
 * to "clean" on the stream before the kernels. d_loc, the matrix as the
 * mismatch branch reads it (device bytes): [rows][k] coefficients, then per
 * column its first row with a non-zero coefficient and that coefficient's
 * inverse. */
int isal_hip_launch_locate_batch(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_tbl, int len,
                                 int k, int rows, long long nstripes, const isal_hip_encmask *em,
                                 const unsigned char *d_loc, unsigned *verdict, void *stream);

/* Ragged (ec_kernels.hip ec_encode_rag / ec_verify_rag): the batch encode and
 * verify where stripe s has its own shard length d_lens[s] (device, nstripes
 * ints). Pointer rows are k sources then rows outputs (stride ptr_stride,
 * every pointer 16-byte aligned); d_tbl is one encode's tables. The work
 * items come from device tables of {stripe, tile} word pairs as
 * isal_hip_ragged_items builds them, one per tile size: passes of at most
 * ISAL_HIP_RAGGED_SMALL_ROWS rows encode ISAL_HIP_RAGGED_TILE_SMALL-byte tiles
 * (d_items_small, which may be NULL when rows has no such pass), every other
 * pass and the verify ISAL_HIP_RAGGED_TILE-byte tiles. One launch per pass;
 * nothing is enqueued when nitems == 0. bad: as isal_hip_launch_verify_batch. */
#define ISAL_HIP_RAGGED_TILE 4096
#define ISAL_HIP_RAGGED_TILE_SMALL 2048
#define ISAL_HIP_RAGGED_SMALL_ROWS 2
#define ISAL_HIP_RAGGED_MAX_ITEMS (1u << 30) /* ec_device.h kMaxItems */
/* the item tables of an object, by tile size */
enum { TILE_BIG, TILE_SMALL, NTILES };
static inline int
isal_hip_tile_bytes(int t)
{
        return t == TILE_SMALL ? ISAL_HIP_RAGGED_TILE_SMALL : ISAL_HIP_RAGGED_TILE;
}
/* whether some pass of an encode of `rows` rows runs the small tile: only the
 * last pass can be short */
static inline int
isal_hip_uses_small_tile(int rows)
{
        const int last = rows % EC_MAX_ROWS_PER_PASS;
        return last >= 1 && last <= ISAL_HIP_RAGGED_SMALL_ROWS;
}
int isal_hip_launch_encode_ragged(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_tbl,
                                  const int *d_lens, const unsigned *d_items, unsigned nitems,
                                  const unsigned *d_items_small, unsigned nitems_small, int k, int rows,
                                  void *stream);
int isal_hip_launch_verify_ragged(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_tbl,
                                  const int *d_lens, const unsigned *d_items, unsigned nitems, int k,
                                  int rows, long long nstripes, unsigned long long *bad, void *stream);
/* Ragged scrub (ec_kernels.hip ec_locate_rag): isal_hip_launch_locate_batch
 * where stripe s has its own length d_lens[s], over the
 * ISAL_HIP_RAGGED_TILE-byte item table (one pass: 2 <= rows <=
 * EC_MAX_ROWS_PER_PASS, always the plain lookup form). verdict (device,
 * nstripes words) is set to "clean" on the stream, then one launch of nitems
 * workgroups; nothing is enqueued when nitems == 0. d_loc as for
 * isal_hip_launch_locate_batch. */
int isal_hip_launch_locate_ragged(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_tbl,
                                  const int *d_lens, const unsigned *d_items, unsigned nitems, int k,
                                  int rows, long long nstripes, const unsigned char *d_loc,
                                  unsigned *verdict, void *stream);

/* Ragged repair (ec_kernels.hip ec_repair_rag): one count class of
 * isal_hip_repair_create_ragged, the rows that lost `rows` shards. Pointer rows
 * are k survivors then rows destinations (stride ptr_stride, every pointer
 * 16-byte aligned); row r has length d_lens[r] and takes the coefficient
 * tables at d_tbl + d_pat[r] dwords, laid out like one encode's tables. Items
 * are {row, tile} pairs as for isal_hip_launch_encode_ragged, and so are the
 * tile sizes: either table may be NULL when rows has no pass of its size. One
 * launch per pass; nothing is enqueued when both item counts are 0. */
int isal_hip_launch_repair_ragged(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_pat,
                                  const uint32_t *d_tbl, const int *d_lens, const unsigned *d_items,
                                  unsigned nitems, const unsigned *d_items_small, unsigned nitems_small,
                                  int k, int rows, void *stream);

/* Ragged overwrite (ec_kernels.hip ec_overwrite_rag): isal_hip_launch_overwrite
 * where stripe s has its own length d_lens[s] and its own count d_nw[s] <=
 * max_nw. Pointer rows are max_nw old shards, max_nw new ones, then rows parity
 * rows (ptr_stride = 2 * max_nw + rows, every live pointer 16-byte aligned);
 * d_idx rows are max_nw words; the entries from d_nw[s] on are zero and never
 * read. Items are {stripe, tile} pairs of the ISAL_HIP_RAGGED_TILE_SMALL-byte
 * tile, none for a stripe without a byte or a slot. One launch per pass,
 * commit as for isal_hip_launch_overwrite; nothing is enqueued when nitems
 * == 0. */
int isal_hip_launch_overwrite_ragged(const uint64_t *d_ptrs, int ptr_stride, const uint32_t *d_idx,
                                     const uint32_t *d_tbl, const int *d_lens, const int *d_nw,
                                     const unsigned *d_items, unsigned nitems, int k, int rows, int max_nw,
                                     int commit, void *stream);

/* Kernel registry (isal_hip_selftest_kernels): every kernel a launcher can
 * launch registers its host handle and a name when the library loads
 * (ec_device.h ISAL_LAUNCH). */
void isal_hip_kreg_add(const void *fn, const char *name);

/* Launch counter shared by the shim and the launchers. */
void isal_hip_count_launch(void);

/* ---- environment knobs (isal_hip_knobs.c): read once, -1 when unset ------- */
enum {
        ISAL_HIP_KNOB_BACKEND,       /* auto(0) | gpu(1) | cpu(2); -2 = unknown word */
        ISAL_HIP_KNOB_CPU_MAX_BYTES, /* auto route: host calls up to this many bytes run on the CPU */
        ISAL_HIP_KNOB_LOG,           /* 1: log every drop-in call's route to stderr, 2: + vector encode kernels */
        ISAL_HIP_KNOB_CPU_SIMD,      /* CPU route width cap: 0 per byte, 1 AVX2, 2 GFNI (tests) */
        ISAL_HIP_KNOB_STAGE_MB,      /* HBM staging per host call (MiB) */
        ISAL_HIP_KNOB_ENC_GLDS,      /* 0: wide encode passes (5-8 rows) load through registers, not the LDS-DMA ring */
        ISAL_HIP_KNOB_CRC_TILES,     /* 4 KiB tiles per CRC workgroup (tests: block geometry) */
        ISAL_HIP_KNOB_CRC_XROWS,     /* 0: fused checksums compute 0/1 parity rows too (tests: no derivation) */
        ISAL_HIP_KNOB_FAULT,         /* fault-injection site of GPU-routed calls (tests) */
        ISAL_HIP_KNOB_FAULT_CHUNK,   /* ... only in this column chunk of a call (tests; unset: every chunk) */
        ISAL_HIP_KNOB_CHUNK_KB,      /* column-chunk bytes per shard of large host calls (pipelined) */
        ISAL_HIP_KNOB_PIPE_CHUNKS,   /* 0: large host calls one chunk at a time (no copy overlap) */
        ISAL_HIP_KNOB_PINNED_DIRECT, /* 0: stage page-locked host shards like pageable ones */
        ISAL_HIP_KNOB_CPU_MAX_BYTES_PINNED, /* auto route limit when every host shard is page-locked */
        ISAL_HIP_KNOB_PAR_COPY,      /* 0: one thread issues a staged call's copies (no helper) */
        ISAL_HIP_KNOB_ENC_XOR,       /* 0: the encode computes 0/1 rows and columns with lookups too */
        ISAL_HIP_KNOB_ENC_LDS,       /* encode low table halves from LDS: 1 always, 0 never (default: 5-6 looked-up rows) */
        ISAL_HIP_KNOB_KARG,          /* 0: device-resident drop-in encodes upload their arguments */
        ISAL_HIP_KNOB_MAX_HELPERS,   /* copy-out helper threads per process (default 8) */
        ISAL_HIP_KNOB_KARG_DONE,     /* 0: kernel-argument calls wait in hipStreamSynchronize (no host mailbox) */
        ISAL_HIP_KNOB_ENC_GROUP,     /* 12/10/8/6/5/4: encode load group forced (tests: every group path) */
        ISAL_HIP_KNOB_KARG_NARROW,   /* drop-in kernel-argument encode with 4-byte lanes: 1 on, 0 off */
        ISAL_HIP_KNOB_ENC_WIDE5,     /* 0: 6-8 row passes keep the largest load group (no groups of 5) */
        ISAL_HIP_KNOB_ENC_LDSX,      /* 0: wide passes compute products with v_perm, not LDS product tables */
        ISAL_HIP_KNOB_COUNT
};
long long isal_hip_knob(int id);
/* bumped by every isal_hip_config_reload(): caches derived from knobs check it */
unsigned isal_hip_knob_generation(void);

/* Fault injection (tests): ISAL_HIP_FAULT=<site> makes the HIP call at that
 * site fail as if it had returned an error, without issuing it — the code
 * after the failure then runs for real. Sites 1-5 are those of every
 * GPU-routed drop-in call (isal_hip_stage.c and isal_hip_karg.c; the fallback
 * paths then run, isal_hip_finish_on_cpu);
 * 6-7 those of isal_hip_batch_set_tables (isal_hip_batch.c). Sites: */
enum {
        FAULT_NONE = 0,
        FAULT_ALLOC = 1,  /* staging / argument buffer allocation */
        FAULT_H2D = 2,    /* a host-to-device copy */
        FAULT_LAUNCH = 3, /* the kernel launch */
        FAULT_D2H = 4,    /* the device-to-host copy of output row 1 (chunked) or of the outputs */
        FAULT_SYNC = 5,   /* the final stream synchronisation */
        FAULT_LDSX_ALLOC = 6, /* a batch's LDS product tables: their device allocation (tolerated:
                           * the batch runs without them) */
        FAULT_LDSX_H2D = 7,   /* ... their upload (the replacement fails, the batch keeps its tables) */
};

/* ---- the host (CPU) route (ec_cpu.c) ---------------------------------------
 * Same ops and return value as isal_hip_run, over HOST-resident shards only,
 * for columns [c0, len): the drop-in calls' route for small host calls, for
 * ISAL_HIP_BACKEND=cpu, for hosts without a GPU, and the fallback when a HIP
 * call fails mid-way (columns before c0 are already final). */
unsigned long long isal_cpu_run(int op, long long c0, int len, int k, int rows, int vec_i,
                                const unsigned char *gftbls, unsigned char *const *src, int nsrc,
                                unsigned char *const *dst);

/* ---- CRC32C of shards (crc_host.c, crc_kernels.hip) -------------------------
 * crc32_iscsi semantics (reference crc/crc_base.c:205-219). Each workgroup
 * covers `tt` consecutive 4 KiB tiles of one shard; lane L owns bytes
 * [16L, 16L+16) of every tile and chains its chunks with Z^4096, leaving one
 * partial per (shard, block, lane):
 *   part[((shard * nblk) + blk) * 256 + L]   (shard = stripe * nshard_total + i)
 * and, when len % 4096 != 0, the crc of its chunk of the last (ragged) tile:
 *   tail[shard * 256 + L]
 * crc32c_combine joins them with the constants of isal_hip_crc32c_plan. */
#define ISAL_HIP_CRC_TILE 4096
#define ISAL_HIP_CRC_SLICES 16
/* Kernel lookup tables (isal_hip_crc32c_tables), all indexed by 5-bit fields
 * so that one table fills the 32 LDS banks exactly once: a wave's lookups
 * into it never bank-conflict (random byte-indexed tables conflict ~3-way).
 * Each dword of a 16-byte chunk splits into 7 fields, bits [0,5) [5,10)
 * [10,15) [15,20) [20,25) [25,30) [30,32):
 *   [0, 256)                     T0: crc of one byte (bytewise tail loop)
 *   [256 + (d*7 + f)*32 + v]     crc(0, chunk) of field f of dword d = v
 *   [256 + 896 + f*32 + v]       Z^4096 of field f of the chain value = v */
#define ISAL_HIP_CRC_FIELDS 7
#define ISAL_HIP_CRC_CHUNK_TAB 256
#define ISAL_HIP_CRC_SHIFT_TAB (ISAL_HIP_CRC_CHUNK_TAB + 4 * ISAL_HIP_CRC_FIELDS * 32)
#define ISAL_HIP_CRC_TAB_DWORDS (ISAL_HIP_CRC_SHIFT_TAB + ISAL_HIP_CRC_FIELDS * 32)
#define ISAL_HIP_CRC_CHUNK_DWORDS (4 * ISAL_HIP_CRC_FIELDS * 32)
/* The combine plan (isal_hip_crc32c_plan, read by crc32c_combine) follows the
 * base tables, at ISAL_HIP_CRC_TAB_DWORDS: the only part of the device image
 * that depends on the length and the block geometry. Offsets within it: */
#define ISAL_HIP_CRC_PLAN_BLOCK 0   /* byte tables of x^(8*4096*tt) */
#define ISAL_HIP_CRC_PLAN_LAST 1024 /* byte tables of x^(8*4096*nfull_last) */
#define ISAL_HIP_CRC_PLAN_W 2048    /* W[L], 256 lanes */
#define ISAL_HIP_CRC_PLAN_CT 2304   /* Ct[L], 256 lanes */
#define ISAL_HIP_CRC_PLAN_XLEN 2560 /* x^(8*len), then 3 words of padding */
#define ISAL_HIP_CRC_PLAN_DWORDS (ISAL_HIP_CRC_PLAN_XLEN + 4)
/* Byte-position tables of the fused kernel's byte path, after the plan:
 *   P:  table p (byte p of a 16-byte chunk) = crc of byte b followed by
 *       15 - p zero bytes, 16 x 256 dwords;
 *   P': the same followed by 4080 more zero bytes (Z^4080 o P: the step of a
 *       pre-shifted chain, crc_kernels.hip). */
#define ISAL_HIP_CRC_B16_TAB (ISAL_HIP_CRC_TAB_DWORDS + ISAL_HIP_CRC_PLAN_DWORDS)
#define ISAL_HIP_CRC_B16_DWORDS (2 * 16 * 256)
void isal_hip_crc32c_byte_tables(uint32_t *out);
/* F' = Z^4080 o crc(0, chunk) as field tables (the layout of CHUNK_TAB), for
 * the checksum-only kernel's pre-shifted chains. */
#define ISAL_HIP_CRC_FPRE_TAB (ISAL_HIP_CRC_B16_TAB + ISAL_HIP_CRC_B16_DWORDS)
#define ISAL_HIP_CRC_FPRE_DWORDS ISAL_HIP_CRC_CHUNK_DWORDS
void isal_hip_crc32c_pre_tables(const uint32_t *tabs, uint32_t *out);
/* The whole device image: base tables, plan, B16, F'. isal_hip_crc32c_image
 * builds all of it for shards of len bytes at tt tiles per workgroup;
 * isal_hip_crc32c_image_len only the part that depends on len and tt (the
 * plan), at its place in out — as isal_hip_crc64_len_tables does for CRC64. */
#define ISAL_HIP_CRC_IMAGE_DWORDS (ISAL_HIP_CRC_FPRE_TAB + ISAL_HIP_CRC_FPRE_DWORDS)
void isal_hip_crc32c_image(long long len, int tt, uint32_t *out);
void isal_hip_crc32c_image_len(long long len, int tt, uint32_t *out);
#define ISAL_HIP_CRC_MAX_FUSED_K 64 /* fused encode keeps k source partials in LDS */

typedef struct {
        long long nfull;  /* full 4 KiB tiles */
        int tail;         /* bytes in the ragged last tile (0: none) */
        long long ntiles; /* nfull + (tail != 0) */
        int tt;           /* tiles per workgroup */
        long long nblk;   /* workgroups per shard */
        long long nfull_last; /* full tiles in the last workgroup */
} isal_hip_crc_geom;

/* ---- ragged CRC32C (isal_hip_ragged_crc; crc_kernels.hip crc32c_shards_rag,
 * crc32c_combine_rag) ---------------------------------------------------------
 * Stripe s has its own shard length lens[s]; the block size tt (tiles per
 * workgroup) is one per object. Stripe s has ceil(ceil(lens[s]/4096)/tt)
 * blocks, and the item table isal_hip_ragged_items(nstripes, lens, 4096*tt)
 * lists them as {stripe, block}; first[s] (nstripes + 1 words) is the row of
 * stripe s's block 0. A work item of the pass is (row w of that table, shard
 * i < nsh = k + rows); it leaves
 *   part[(w * nsh + i) * 256 + L]          the chain of lane L over the block's
 *                                          full tiles
 *   tail[(stripe * nsh + i) * 256 + L]     the crc of lane L's chunk of the
 *                                          ragged tile (lens[s] % 4096 != 0)
 * The image (isal_hip_crc32c_ragged_image) depends on tt alone:
 *   [0, TAB_DWORDS)   isal_hip_crc32c_tables (T0, F, Z^4096)
 *   RAG_FPRE          F' (isal_hip_crc32c_pre_tables)
 *   RAG_BLOCK         byte tables of x^(8*4096*tt)       (Horner across blocks)
 *   RAG_X             X[n] = x^(8n), n < 8192            (W, Ct, the tail of x^(8*len))
 *   RAG_SQ            x^(8*4096*2^i), i < 19             (x^(8*len) by square-and-multiply:
 *                                                         len < 2^31 has fewer than 2^19 tiles)
 *   RAG_PW            x^(8*4096*j), j = 0..tt            (the last block's full tiles) */
#define ISAL_HIP_CRC_RAG_FPRE ISAL_HIP_CRC_TAB_DWORDS
#define ISAL_HIP_CRC_RAG_BLOCK (ISAL_HIP_CRC_RAG_FPRE + ISAL_HIP_CRC_FPRE_DWORDS)
#define ISAL_HIP_CRC_RAG_X (ISAL_HIP_CRC_RAG_BLOCK + 1024)
#define ISAL_HIP_CRC_RAG_X_DWORDS (2 * ISAL_HIP_CRC_TILE)
#define ISAL_HIP_CRC_RAG_SQ (ISAL_HIP_CRC_RAG_X + ISAL_HIP_CRC_RAG_X_DWORDS)
#define ISAL_HIP_CRC_RAG_NSQ 19
#define ISAL_HIP_CRC_RAG_SQ_DWORDS 32 /* a wave's lanes 0..31 read one word each */
#define ISAL_HIP_CRC_RAG_PW (ISAL_HIP_CRC_RAG_SQ + ISAL_HIP_CRC_RAG_SQ_DWORDS)
#define ISAL_HIP_CRC_RAG_MAX_TT 1024 /* ISAL_HIP_CRC_TILES is clamped to this */
/* What the first checksum call of one width allocates on a ragged object
 * (isal_hip_ragged_crc.c): the block size it picked, the {stripe, block} item
 * table with its per-stripe prefix first[], and the partials, one word of the
 * width per (item, shard, lane). d_part != NULL: set up. */
typedef struct {
        int tt;
        unsigned nitems;
        unsigned *d_items, *d_first;
        void *d_part;
} isal_hip_ragged_ck;
void isal_hip_ragged_ck_drop(isal_hip_ragged_ck *ck);

/* The ragged batch object (isal_hip_ragged.c; its checksum state is
 * isal_hip_ragged_crc.c's). */
struct isal_hip_ragged {
        int k, rows, nstripes, device;
        unsigned nitems[NTILES];
        uint64_t *d_ptrs;
        uint32_t *d_tbl;
        int *d_lens;
        unsigned *d_items[NTILES];
        /* the checksums' own state (isal_hip_ragged_crc): the lengths as
         * create saw them, then what the first checksum call allocates */
        int *h_lens;
        isal_hip_ragged_ck ck32;  /* CRC32C: its partials are followed by the tail rows, d_tail */
        uint32_t *d_crc, *d_tail; /* CRC32C's image (set: CRC32C is set up) */
        /* CRC64's own: block size, item table and partials from its first
         * call, one image per variant from the first call with that variant */
        isal_hip_ragged_ck ck64;
        uint64_t *d_c64image[8]; /* ISAL_HIP_CRC64_NVARIANTS */
        /* the sector checksums' own (isal_hip_sector_crc.c): one image per
         * flavour and one table of first sectors per sector size, each from the
         * first call that needs it */
        uint32_t *d_sec32;
        uint64_t *d_sec64[8];
        unsigned long long *d_sec_first[4]; /* ISAL_HIP_SECTOR_NSIZES */
        uint32_t *d_sec16; /* the T10 guard's image (isal_hip_dif.c), from its first call */
};
/* isal_hip_ragged_encode's body, for a caller already on the object's device */
int isal_hip_ragged_encode_on_device(struct isal_hip_ragged *r, void *stream);
size_t isal_hip_crc32c_ragged_image_dwords(int tt);
void isal_hip_crc32c_ragged_image(int tt, uint32_t *out);
/* One launch over nitems * nsh work items (at most ISAL_HIP_RAGGED_MAX_ITEMS:
 * hipErrorInvalidValue past it, nothing enqueued); nothing when nitems == 0. */
int isal_hip_launch_crc_ragged(const uint64_t *d_ptrs, int nsh, const int *d_lens, const unsigned *d_items,
                               unsigned nitems, int tt, const uint32_t *d_image, uint32_t *d_part,
                               uint32_t *d_tail, void *stream);
/* out[stripe * nsh + i] = crc32_iscsi(shard, lens[stripe], init); init for a
 * stripe of length 0. One launch. */
int isal_hip_launch_crc_combine_ragged(const uint32_t *d_part, const uint32_t *d_tail, const uint32_t *d_image,
                                       const int *d_lens, const unsigned *d_first, int nsh, int tt,
                                       unsigned int init, uint32_t *out, long long nstripes, void *stream);

/* ---- ragged CRC64 (isal_hip_ragged_crc64; crc64_kernels.hip crc64_shards_rag,
 * crc64_combine_rag) ----------------------------------------------------------
 * The geometry is the ragged CRC32C's: tt tiles per block, one value per
 * object; stripe s has ceil(ceil(lens[s]/4096)/tt) blocks, listed as {stripe,
 * block} by isal_hip_ragged_items(nstripes, lens, 4096*tt), and first[s] is
 * the row of stripe s's block 0. As in the uniform CRC64 the pass covers the
 * FULL tiles only: work item (row w, shard i < nsh) leaves
 *   part[(w * nsh + i) * 256 + L]   the chain of lane L over the block's full
 *                                   tiles (0 for a last block without one)
 * and the combine reads the bytes after the last full tile from the shard.
 * The uniform batch applies Z^(4096*nfull_last), Z^(16*(tail/16)) and Z^len as
 * maps tabulated on the host for one length; here they are products in the
 * flavour's quotient ring (crc64_host.c isal_hip_crc64_mulmod; on the device a
 * 64-step shift-and-XOR) of elements that depend on no length. The image
 * (isal_hip_crc64_ragged_image, uint64 entries) depends on (variant, tt) alone:
 *   RAG_BYTE   reference byte table (the last len % 16 bytes)
 *   RAG_CHUNK  raw(0, 16-byte chunk)                     (the tail's chunks)
 *   RAG_BLOCK  field tables of Z^(4096*tt)               (Horner across blocks)
 *   RAG_TREE   Z^(16 * 2^s), s = 0..7                    (wave_fold)
 *   (crc64_combine_rag keeps BYTE..TREE in LDS: RAG_COMBINE_ENTRIES)
 *   RAG_PRE    F_u, F'_u of the pre-shifted chains       (all the pass reads)
 *   RAG_X      X[n] = x^(8n), n < 4096: X[16 * q] shifts the full tiles past the
 *              tail's chunks, X[len % 4096] is the low part of x^(8*len). (Every
 *              index is below one tile: the CRC32C image needs two for its
 *              per-lane W[L]; here wave_fold moves the lanes.)
 *   RAG_SQ     x^(8*4096*2^i), i < 19, then 1s up to 32  (x^(8*len) by a wave
 *                                                         product over the set bits of nfull)
 *   RAG_PW     x^(8*4096*j), j = 0..tt                   (the last block's full tiles)
 * No Z^4096 table (SHIFT_TAB): only the byte-load kernel of unaligned shards
 * steps with it, and a ragged batch's shards are 16-byte aligned. */
#define ISAL_HIP_CRC64_RAG_BYTE 0
#define ISAL_HIP_CRC64_RAG_CHUNK 256
#define ISAL_HIP_CRC64_RAG_BLOCK (ISAL_HIP_CRC64_RAG_CHUNK + ISAL_HIP_CRC64_CHUNK_ENTRIES)
#define ISAL_HIP_CRC64_RAG_TREE (ISAL_HIP_CRC64_RAG_BLOCK + ISAL_HIP_CRC64_OP_ENTRIES)
#define ISAL_HIP_CRC64_RAG_COMBINE_ENTRIES (ISAL_HIP_CRC64_RAG_TREE + 8 * ISAL_HIP_CRC64_OP_ENTRIES)
#define ISAL_HIP_CRC64_RAG_PRE ISAL_HIP_CRC64_RAG_COMBINE_ENTRIES
#define ISAL_HIP_CRC64_RAG_X (ISAL_HIP_CRC64_RAG_PRE + 2 * ISAL_HIP_CRC64_CHUNK_ENTRIES)
#define ISAL_HIP_CRC64_RAG_X_ENTRIES ISAL_HIP_CRC_TILE
#define ISAL_HIP_CRC64_RAG_SQ (ISAL_HIP_CRC64_RAG_X + ISAL_HIP_CRC64_RAG_X_ENTRIES)
#define ISAL_HIP_CRC64_RAG_NSQ 19
#define ISAL_HIP_CRC64_RAG_SQ_ENTRIES 32 /* a wave's lanes read entry lane % 32 */
#define ISAL_HIP_CRC64_RAG_PW (ISAL_HIP_CRC64_RAG_SQ + ISAL_HIP_CRC64_RAG_SQ_ENTRIES)
size_t isal_hip_crc64_ragged_image_entries(int tt);
void isal_hip_crc64_ragged_image(int variant, int tt, uint64_t *out);
/* a * b and x^(8n) in the variant's quotient ring, registers in the variant's
 * bit order; ring_poly: P(x) without x^64 in that order */
uint64_t isal_hip_crc64_mulmod(int variant, uint64_t a, uint64_t b);
uint64_t isal_hip_crc64_xpow8n(int variant, unsigned long long n);
uint64_t isal_hip_crc64_ring_poly(int variant);
/* One launch over nitems * nsh work items (at most ISAL_HIP_RAGGED_MAX_ITEMS:
 * hipErrorInvalidValue past it, nothing enqueued); nothing when nitems == 0. */
int isal_hip_launch_crc64_ragged(const uint64_t *d_ptrs, int nsh, const int *d_lens, const unsigned *d_items,
                                 unsigned nitems, int tt, int refl, const uint64_t *d_image, uint64_t *d_part,
                                 void *stream);
/* out[stripe * nsh + i] = crc64_<variant>(init, shard, lens[stripe]); init for
 * a stripe of length 0. poly = isal_hip_crc64_ring_poly(variant). One launch. */
int isal_hip_launch_crc64_combine_ragged(const uint64_t *d_part, const uint64_t *d_ptrs, const uint64_t *d_image,
                                         const int *d_lens, const unsigned *d_first, int nsh, int tt, int refl,
                                         uint64_t poly, uint64_t init, uint64_t *out, long long nstripes,
                                         void *stream);

/* Tiles per CRC workgroup (CRC32C and CRC64) of a launch over nstripes
 * stripes of len-byte shards: def, halved for small launches;
 * ISAL_HIP_CRC_TILES overrides (isal_hip_batch.c). */
int isal_hip_crc_tiles(int len, int nstripes, int def);

/* ---- CRC64 of shards (crc64_host.c, crc64_kernels.hip) ---------------------
 * The eight crc64_* flavours (reference include/crc64.h:54-163). Same lane
 * layout as CRC32C: crc64_shards leaves one 64-bit chain per (shard, block,
 * lane) over the FULL 4 KiB tiles, part[(shard * nblk + blk) * 256 + L];
 * crc64_combine folds them, adds the ragged tail read straight from the shard
 * and the init term. Table buffer (uint64 entries, one per variant and
 * geometry), every map as 14 field tables of 32 entries (crc64_host.c):
 *   BYTE_TAB   reference byte table (tail bytes)
 *   CHUNK_TAB  raw(0, 16-byte chunk), 4 dwords x 7 fields x 32
 *   SHIFT_TAB  Z^4096                      } crc64_shards loads CHUNK..SHIFT
 *   OP_BLOCK   Z^(4096*tt)   OP_LAST Z^(4096*nfull_last)
 *   OP_TREE    Z^(16 * 2^s), s = 0..7 (lane tree)   OP_TAIL Z^(16*(tail/16))
 *   (crc64_combine loads BYTE..OP_TAIL: COMBINE_ENTRIES)
 *   SLICE_TAB  slicing-by-8 tables of the fused kernel's byte-indexed chunk
 *              path, in the "u-domain" u = pi(s) (pi = byte swap for the norm
 *              flavours, identity for refl), where processing 8 bytes d is
 *              u' = A(d ^ u) for every flavour:
 *                A_j[v]  = pi(raw(0, v at byte j of 8)),  8 x 256
 *                A'_j[v] = pi(Z^4080 raw(0, v at byte j of 8)), 8 x 256
 *              (A' advances a lane's chain past the rest of its tile) */
#define ISAL_HIP_CRC64_OP_ENTRIES (2 * ISAL_HIP_CRC_FIELDS * 32)
#define ISAL_HIP_CRC64_BYTE_TAB 0
#define ISAL_HIP_CRC64_CHUNK_TAB 256
#define ISAL_HIP_CRC64_SHIFT_TAB (ISAL_HIP_CRC64_CHUNK_TAB + 4 * ISAL_HIP_CRC_FIELDS * 32)
#define ISAL_HIP_CRC64_OP_BLOCK (ISAL_HIP_CRC64_SHIFT_TAB + ISAL_HIP_CRC64_OP_ENTRIES)
#define ISAL_HIP_CRC64_OP_LAST (ISAL_HIP_CRC64_OP_BLOCK + ISAL_HIP_CRC64_OP_ENTRIES)
#define ISAL_HIP_CRC64_OP_TREE (ISAL_HIP_CRC64_OP_LAST + ISAL_HIP_CRC64_OP_ENTRIES)
#define ISAL_HIP_CRC64_OP_TAIL (ISAL_HIP_CRC64_OP_TREE + 8 * ISAL_HIP_CRC64_OP_ENTRIES)
#define ISAL_HIP_CRC64_COMBINE_ENTRIES (ISAL_HIP_CRC64_OP_TAIL + ISAL_HIP_CRC64_OP_ENTRIES)
#define ISAL_HIP_CRC64_CHUNK_ENTRIES (4 * ISAL_HIP_CRC_FIELDS * 32)
#define ISAL_HIP_CRC64_SLICE_TAB ISAL_HIP_CRC64_COMBINE_ENTRIES
#define ISAL_HIP_CRC64_SLICE_ENTRIES (2 * 8 * 256)
/*   PRE_TAB    field tables of the checksum-only kernel's pre-shifted chains
 *              (u-domain): F_u = pi o raw(0, chunk), F'_u = pi o Z^4080 o raw(0, chunk) */
#define ISAL_HIP_CRC64_PRE_TAB (ISAL_HIP_CRC64_SLICE_TAB + ISAL_HIP_CRC64_SLICE_ENTRIES)
#define ISAL_HIP_CRC64_TAB_ENTRIES (ISAL_HIP_CRC64_PRE_TAB + 2 * ISAL_HIP_CRC64_CHUNK_ENTRIES)

typedef struct {
        long long nfull;      /* full 4 KiB tiles */
        int tail;             /* bytes after them (< 4096) */
        int tt;               /* tiles per workgroup */
        long long nblk;       /* workgroups per shard (0 when nfull == 0) */
        long long nfull_last; /* full tiles in the last workgroup */
} isal_hip_crc64_geom;

int isal_hip_crc64_is_refl(int variant);
void isal_hip_crc64_cpu_tables(int variant, uint64_t byte[256], uint64_t slice[8 * 256]);
uint64_t isal_hip_crc64_poly(int variant);

/* ---- the checksum entry points' CPU route (crc_cpu.c): host buffers --------
 * crc32_iscsi semantics (register starts at init, no inversion) and
 * crc64_<variant> semantics (starts at ~init, inverted on return). */
uint32_t isal_cpu_crc32c(uint32_t init, const unsigned char *buf, uint64_t len);
uint64_t isal_cpu_crc64(int variant, uint64_t init, const unsigned char *buf, uint64_t len);
void isal_hip_crc64_geometry(long long len, int tt, isal_hip_crc64_geom *g);
void isal_hip_crc64_zpow(int variant, unsigned long long n, uint64_t out[64]);
void isal_hip_crc64_tables(int variant, long long len, int tt, uint64_t *tabs);
/* only OP_BLOCK, OP_LAST and OP_TAIL (the length / geometry dependent maps) */
void isal_hip_crc64_len_tables(int variant, long long len, int tt, uint64_t *tabs);
uint64_t isal_hip_crc64_init_term(int variant, long long len, uint64_t init);

/* crc64(init, shard, len) of the nsh shards of each stripe (d_ptrs row
 * stride ptr_stride, shards 0..nsh-1) into out[stripe * nsh + i]; init_term =
 * isal_hip_crc64_init_term(variant, len, init). */
int isal_hip_launch_crc64(const uint64_t *d_ptrs, int ptr_stride, int nsh, long long nstripes,
                          int len, int vec16, int refl, int tt, const uint64_t *d_tabs,
                          uint64_t *d_part, uint64_t init_term, uint64_t *out, void *stream);
/* Encode (one pass, rows <= EC_MAX_ROWS_PER_PASS; d_ptrs rows = k sources then
 * rows parity, stride k + rows) and crc64 of all k + rows shards into
 * out[stripe * (k + rows) + i]. Needs 16-byte aligned shards, len % 16 == 0,
 * len >= ISAL_HIP_CRC_TILE and k <= ISAL_HIP_CRC64_MAX_FUSED_K. */
#define ISAL_HIP_CRC64_MAX_FUSED_K 32 /* source chains: k * 2 KiB of LDS */
int isal_hip_launch_encode_crc64(const uint64_t *d_ptrs, int k, int rows, long long nstripes,
                                 int len, const uint32_t *d_tbl, const isal_hip_xrows *xr, int refl,
                                 int tt, const uint64_t *d_tabs, uint64_t *d_part,
                                 uint64_t init_term, uint64_t *out, void *stream);

uint32_t isal_hip_crc32c_mulmod(uint32_t a, uint32_t b);
uint32_t isal_hip_crc32c_xpow8n(unsigned long long n);
void isal_hip_crc32c_tables(uint32_t *tabs);
void isal_hip_crc_geometry(long long len, int tt, isal_hip_crc_geom *g);
void isal_hip_crc32c_plan(long long len, int tt, uint32_t *plan);

/* CRC partials of shards idx0..idx0+nsh-1 of each stripe (no encoding);
 * shard numbering in part/tail starts at shard0 within nshard_total. */
int isal_hip_launch_crc(const uint64_t *d_ptrs, int ptr_stride, int idx0, int nsh,
                        long long nstripes, int len, int vec16, int tt, const uint32_t *d_tabs,
                        uint32_t *d_part, uint32_t *d_tail, int nshard_total, int shard0,
                        void *stream);
/* Encode (as isal_hip_launch_encode) and leave the CRC partials of the k
 * sources (shards 0..k-1) and the rows outputs (shards k..k+rows-1). Needs
 * 16-byte aligned shards, len % 16 == 0 and k <= ISAL_HIP_CRC_MAX_FUSED_K. */
int isal_hip_launch_encode_crc(const uint64_t *d_ptrs, int ptr_stride, int src_idx0, int dst_idx0,
                               const uint32_t *d_tbl, const isal_hip_xrows *xr, int len, int k,
                               int rows, long long nstripes, int tt, const uint32_t *d_tabs,
                               uint32_t *d_part, uint32_t *d_tail, void *stream);
/* out[sh] = crc32_iscsi of shard sh (sh < nsh) from its partials. */
int isal_hip_launch_crc_combine(const uint32_t *d_part, const uint32_t *d_tail,
                                const uint32_t *d_plan, long long nblk, int has_tail,
                                unsigned int init, uint32_t *out, long long nsh, void *stream);

/* ---- sector checksums (isal_hip_sector_crc.c, crc_sector_kernels.hip) -------
 * One word per `sector` bytes of every shard (isal_hip.h "sector checksums"),
 * sector a power of two from ISAL_HIP_SECTOR_MIN to one CRC tile. The device
 * images depend on the flavour alone, never on a length or the sector size:
 *   CRC32C (dwords)   the chunk map, ISAL_HIP_CRC_CHUNK_DWORDS (the layout of
 *                     CHUNK_TAB), then the field tables (the layout of
 *                     SHIFT_TAB) of Z^(16 * 2^d), d = 0 .. ISAL_HIP_SECTOR_NZ - 1
 *   crc64 (entries)   the chunk map, ISAL_HIP_CRC64_CHUNK_ENTRIES, then the 14
 *                     field tables of the same seven maps
 * Z^16 .. Z^512 join the lanes of a wave, Z^1024 the waves of a 2 or 4 KiB
 * sector. */
#define ISAL_HIP_SECTOR_MIN 512
#define ISAL_HIP_SECTOR_NZ 7
#define ISAL_HIP_SECTOR_NSIZES 4 /* 512, 1024, 2048, 4096 */
#define ISAL_HIP_SECTOR32_DWORDS (ISAL_HIP_CRC_CHUNK_DWORDS + ISAL_HIP_SECTOR_NZ * ISAL_HIP_CRC_FIELDS * 32)
#define ISAL_HIP_SECTOR64_ENTRIES (ISAL_HIP_CRC64_CHUNK_ENTRIES + ISAL_HIP_SECTOR_NZ * ISAL_HIP_CRC64_OP_ENTRIES)
void isal_hip_crc32c_sector_image(uint32_t *out);
void isal_hip_crc64_sector_image(int variant, uint64_t *out);
/* Where the nwork (shard, 4 KiB tile) work items of a launch lie. d_ptrs: rows
 * of nsh shard addresses, every one 16-byte aligned. Uniform (d_items NULL):
 * every shard has len bytes in ntiles tiles, item w is tile w % ntiles of shard
 * w / ntiles, whose sector 0 is word (w / ntiles) * ceil(len / sector). Ragged:
 * item w is shard w % nsh of row w / nsh of the {stripe, tile} table d_items
 * (ISAL_HIP_RAGGED_TILE-byte tiles), the stripe's length is d_lens[stripe] and
 * sector 0 of its shard j is word nsh * d_first[stripe] + j * ceil(len / sector)
 * (d_first: isal_hip_ragged_sector_offsets). */
typedef struct {
        const uint64_t *d_ptrs;
        int nsh, sector;
        unsigned long long nwork;
        int len;
        unsigned ntiles;
        const int *d_lens;
        const unsigned *d_items;
        const unsigned long long *d_first;
} isal_hip_sector_geom;
/* One launch, no other: out[word] = crc32_iscsi(sector bytes, n, init) /
 * crc64 of the flavour whose image, direction and ring polynomial
 * (isal_hip_crc64_ring_poly) are given. hipErrorInvalidValue, nothing
 * enqueued, for nwork == 0 or past ISAL_HIP_RAGGED_MAX_ITEMS or a bad sector. */
int isal_hip_launch_sector_crc32c(const isal_hip_sector_geom *g, const uint32_t *d_image, unsigned int init,
                                  uint32_t *out, void *stream);
int isal_hip_launch_sector_crc64(const isal_hip_sector_geom *g, const uint64_t *d_image, int refl, uint64_t poly,
                                 uint64_t init, uint64_t *out, void *stream);
/* What the entry points of isal_hip_sector_crc.c and isal_hip_dif.c share; no
 * HIP call unless stated.
 * _batch_geom / _ragged_geom: ISAL_HIP_EINVAL for a NULL object, a bad sector,
 *   (uniform) an unaligned shard or more work items than one launch takes; 1
 *   when every length is 0 (nothing to do); else 0 with *g filled but for
 *   d_first, which isal_hip_sector_ragged_first uploads at the first call with
 *   that sector size (on the object's device) and sets.
 * _put: *slot = the device copy of the malloc'ed image h (freed here; NULL:
 *   ISAL_HIP_ENOMEM); a failure leaves *slot NULL and no HIP error behind. */
struct isal_hip_batch;
int isal_hip_sector_index(int sector);
int isal_hip_sector_batch_geom(const struct isal_hip_batch *b, int sector, isal_hip_sector_geom *g);
int isal_hip_sector_ragged_geom(const struct isal_hip_ragged *r, int sector, isal_hip_sector_geom *g);
int isal_hip_sector_ragged_first(struct isal_hip_ragged *r, int sector, isal_hip_sector_geom *g);
int isal_hip_sector_put(void *slot, void *h, size_t bytes);

/* ---- T10 protection information (isal_hip_dif.c, crc_sector_kernels.hip) ----
 * The sector pass over a third family, crc16_t10dif: a normal (not reflected)
 * 16-bit register in the low half of a dword, polynomial x^16 + 0x8BB7, bit i
 * the coefficient of x^i. Its image: the chunk map in the layout of CHUNK_TAB
 * (28 field tables of 32 dwords), then for each Z^(16 * 2^d), d = 0 ..
 * ISAL_HIP_SECTOR_NZ - 1, the ISAL_HIP_CRC16_FIELDS field tables of a 16-bit
 * register: bits [0,5) [5,10) [10,15) [15,16). */
#define ISAL_HIP_CRC16_POLY 0x8BB7u
#define ISAL_HIP_CRC16_FIELDS 4
#define ISAL_HIP_CRC16_OP_DWORDS (ISAL_HIP_CRC16_FIELDS * 32)
#define ISAL_HIP_SECTOR16_DWORDS (ISAL_HIP_CRC_CHUNK_DWORDS + ISAL_HIP_SECTOR_NZ * ISAL_HIP_CRC16_OP_DWORDS)
uint32_t isal_hip_crc16_mulmod(uint32_t a, uint32_t b);
uint32_t isal_hip_crc16_xpow8n(unsigned long long n); /* x^(8n) mod P */
void isal_hip_crc16_sector_image(uint32_t *out);
/* What the lane at position 0 of a sector does with its guard g (sector i of
 * shard n = s*m + j, word w of the sector layout):
 *   GUARD     crc[w] = g
 *   GENERATE  the 8 bytes at pi + 8*w = g, app, ref, each most significant
 *             byte first; ref = ref0[n] (0 for a NULL ref0), plus i for type 1
 *   VERIFY    the stored tuple at pi + 8*w against g, app and ref under flags
 *             and the escape rule (isal_hip.h); a failing sector does
 *             atomicMin(bad + n, i << 3 | kinds). */
enum { ISAL_HIP_DIF_GUARD, ISAL_HIP_DIF_GENERATE, ISAL_HIP_DIF_VERIFY };
typedef struct {
        int mode, type;
        unsigned seed, app, flags;
        const unsigned *ref0;
        unsigned short *crc; /* GUARD */
        unsigned char *pi;   /* GENERATE (written), VERIFY (read) */
        unsigned *bad;       /* VERIFY */
} isal_hip_dif_args;
/* One launch, no other (the caller fills bad): hipErrorInvalidValue, nothing
 * enqueued, as for isal_hip_launch_sector_crc32c or for an unknown mode. */
int isal_hip_launch_sector_t10dif(const isal_hip_sector_geom *g, const uint32_t *d_image,
                                  const isal_hip_dif_args *a, void *stream);

/* The uniform batch object (isal_hip_batch.c; its sector checksums are
 * isal_hip_sector_crc.c's). */
struct isal_hip_batch {
        int len, k, rows, nstripes, device, vec16;
        uint64_t *d_ptrs;
        uint32_t *d_tbl;
        isal_hip_xrows xr; /* 0/1 parity rows: CRCs derived, not computed */
        isal_hip_encmask em; /* 0/1 rows and columns: XORs instead of lookups */
        /* CRC32C state, allocated on first use: kernel tables + combine plan,
         * and the per-lane partials (crc_kernels.hip) */
        uint64_t *d_ldsx; /* LDS product tables of the wide passes (NULL: not used) */
        isal_hip_crc_geom crc;
        uint32_t *d_crc, *d_part, *d_tail;
        /* CRC64 state, allocated on first use: one table set per variant
         * and pass used (never overwritten, so switching variants needs no
         * device synchronisation) and the per-lane chains. The fused pass
         * (c64_tt tiles per block) and the checksum-only pass (c64_tt_ck)
         * have their own block geometry; the partials are sized for the
         * shorter blocks. */
        int c64_tt, c64_tt_ck;
        uint64_t *d_c64tab[8], *d_c64tab_ck[8], *d_c64part; /* ISAL_HIP_CRC64_NVARIANTS */
        /* the sector checksums' images, from the first call that needs one */
        uint32_t *d_sec32;
        uint64_t *d_sec64[8];
        uint32_t *d_sec16; /* the T10 guard's image (isal_hip_dif.c), from its first call */
};

#ifdef __cplusplus
}
#endif

#endif /* ISAL_HIP_INTERNAL_H */
