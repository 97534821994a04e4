/* psk_soft_frame.h -- the psk_soft_frame_ family of the C ABI of libpsk_soft_hip.so: byte frames found in and cut from decoded bits
 * on the GPU.  Part of psk_soft_hip.h, which includes it inside its extern "C" block and behind the types it needs
 * (psk_soft_handle_t, psk_soft_status); include psk_soft_hip.h, not this file.  The ABI version is psk_soft_hip.h's and stays 2. */
#ifndef PSK_SOFT_FRAME_H
#define PSK_SOFT_FRAME_H
#ifndef PSK_SOFT_HIP_H
#error "include psk_soft_hip.h, which includes psk_soft_frame.h"
#endif

/* ---- frames as aligned bytes: between the decoder and the outer code ---------------------------------------------------------------
 * The decoder writes a stream of packed bits with no byte alignment; the outer code reads frames of bytes.  Two calls stand
 * between them.  The SEARCH looks for a known word in the decoded bits of a stream -- at every bit offset, in both polarities (a
 * BPSK half-turn leaves the decoder as inverted bits), optionally folded over a period -- and leaves one small record per stream:
 * that record is all that crosses the link.  The CUT writes byte frames that start at any bit of a stream -- aligned, inverted
 * where asked, deinterleaved (the convolutional byte interleaver of DVB, as a gather) and mapped through a 256-byte table (the
 * CCSDS dual basis, a caller's table) -- where the rs call reads them.  Everything is integer arithmetic: the host definitions
 * and the device agree byte for byte.
 *
 * The calls touch no demodulator state, statistics or history, and no other record.  Streams, words and tables are read, never
 * written.
 *
 * Bit order.  Stream bit i of a stream (bits, bit0) is bit 7 - ((bit0 + i) & 7) of byte bits[(bit0 + i) >> 3]: the order
 *   PSK_SOFT_VITERBI_PACKED writes.  `bits` may have any byte alignment.  A kernel may read an aligned dword that holds a stream
 *   bit the call names, nothing further.
 *
 * The search.  A word has L = 1 .. 64 bits; `word` and `care` are uint64 values whose bit L-1-j is word bit j (the first bit in
 *   stream order is the most significant of the L); bits at L and above are zero; C = popcount(care) >= 1.
 *   Windows are p = 0 .. n_bits - L (none when n_bits < L).  d(p) is the number of care positions at which the stream bits
 *   p .. p+L-1 differ from the word.  Window p is a hit of polarity 0 when d(p) <= max_diff and a hit of polarity 1 (inverted) when
 *   C - d(p) <= max_diff; 2 max_diff < C is required, so it is never both.  Its diff is min(d, C - d) and its polarity 0 when
 *   the two are equal.
 *   With period P = 1 .. 2^20 the phase of p is p mod P and score[phase] the number of hits of either polarity at it; the best
 *   phase has the greatest score, the smallest phase on a tie.  With P = 0 there is no fold.
 *   Record: n_hit per polarity; min_diff / min_pos / min_pol, the smallest diff over all windows, the smallest position on a tie;
 *   best_phase / best_score / best_inv (hits of polarity 1 at the best phase), zero with P = 0; hits[0 .. n_listed-1]: with P = 0
 *   the first 16 hits of the stream in position order, with P > 0 the first 16 hits AT THE BEST PHASE (their polarities say which
 *   packet of eight carries DVB's inverted byte, and whether the whole stream is inverted).  A stream without windows has
 *   everything but flags, length and n_windows zero.
 *   Cost.  One stream's fold occupies ceil(min(P, n_windows) / tile) workgroups of one wave (psk_soft_frame_tile phases each;
 *   with P = 0 tiles of 256 tile windows): a call is fast with many streams and slow with one.
 *
 * The cut.  A format has B = 1 .. 255 branches of cell M = 0 .. 255 with B (B-1) M <= 2^24 (B = 1 or M = 0: no interleaver) and an
 *   optional table T of 256 bytes (NULL: the identity).  Stream byte S(q), q >= 0, is the stream bits bit + 8q .. bit + 8q + 7,
 *   the first most significant.  out[i] = T[S(i + ((branch0 + i) mod B) M B) ^ (INVERT ? 0xff : 0)] for i < n_bytes: the Forney
 *   deinterleaver as a gather.  A transmitter delays branch j by j M cells = j M B stream bytes; branch 0 (the sync byte's) is
 *   not delayed, so a cut that starts where the search found the sync byte returns the packet as it was before the interleaver.
 *   Exactly n_bytes are written and no byte outside them.  The outputs of a call may overlap neither each other nor any input:
 *   the caller's duty, not checked.
 *   Record: flags, n_bytes, span (the stream bytes from `bit` the frame touches: 1 + the greatest source index) and n_ones, the
 *   one-bits of the bytes written (a dead stream shows as 0 or 8 n_bytes). */
#define PSK_SOFT_FRAME_SLOTS        16
#define PSK_SOFT_FRAME_MAX_STREAMS  (1u << 20)
#define PSK_SOFT_FRAME_MAX_FRAMES   (1u << 20)
#define PSK_SOFT_FRAME_MAX_PERIOD   (1u << 20)
#define PSK_SOFT_FRAME_MAX_BITS     (1u << 31)
#define PSK_SOFT_FRAME_MAX_BYTES    (1u << 20)
#define PSK_SOFT_FRAME_MAX_DELAY    (1u << 24)   /* B (B-1) M */
#define PSK_SOFT_FRAME_HITS         16
enum { PSK_SOFT_FRAME_INVERT = 1 };  /* psk_soft_frame_cut_in_t.flags */
/* the records' flags: DATA or PLANNED; in the cut's ORed with the frame's flags shifted left by one */
enum { PSK_SOFT_FRAME_DATA = 1, PSK_SOFT_FRAME_REC_INVERT = 2, PSK_SOFT_FRAME_PLANNED = 128 };

typedef struct psk_soft_frame_search_in {
    const uint8_t *bits;  /* DEVICE pointer, any alignment; NULL: the stream is skipped                                        */
    uint64_t bit0;        /* the bit of `bits` at which the stream starts                                                     */
    uint32_t n_bits;      /* 1 .. 2^31                                                                                       */
    uint32_t word;        /* 1 + the slot of the word; 0: the stream is skipped                                              */
    uint32_t max_diff;    /* 2 max_diff < popcount(care)                                                                     */
    uint32_t period;      /* 0: no fold; 1 .. 2^20                                                                           */
    uint32_t flags;       /* none defined: zero                                                                              */
    uint32_t pad[3];      /* zero                                                                                            */
} psk_soft_frame_search_in_t;  /* 48 bytes */

typedef struct psk_soft_frame_hit {
    uint32_t pos;         /* the window's first stream bit                                                                   */
    uint16_t diff;
    uint8_t pol;          /* 1: inverted                                                                                     */
    uint8_t zero;
} psk_soft_frame_hit_t;   /* 8 bytes */

typedef struct psk_soft_frame_search {   /* one per stream of the LAST search call; the offsets are stated, the tests pin them */
    uint32_t flags;                      /*   0  PSK_SOFT_FRAME_DATA or _PLANNED                                            */
    uint32_t length;                     /*   4  L                                                                          */
    uint32_t n_windows;                  /*   8                                                                             */
    uint32_t n_hit[2];                   /*  12  per polarity                                                               */
    uint32_t min_diff;                   /*  20                                                                             */
    uint32_t min_pos;                    /*  24                                                                             */
    uint32_t min_pol;                    /*  28                                                                             */
    uint32_t best_phase;                 /*  32                                                                             */
    uint32_t best_score;                 /*  36                                                                             */
    uint32_t best_inv;                   /*  40                                                                             */
    uint32_t n_listed;                   /*  44  0 .. 16                                                                    */
    uint32_t pad[4];                     /*  48  zero                                                                       */
    psk_soft_frame_hit_t hits[16];       /*  64  the entries from n_listed on are zero                                      */
} psk_soft_frame_search_t;               /* 192 bytes */

typedef struct psk_soft_frame_cut_in {
    const uint8_t *bits;  /* DEVICE pointer, any alignment; NULL: the frame is skipped                                         */
    uint64_t bit;         /* the bit of `bits` at which the frame starts                                                     */
    uint8_t *out;         /* DEVICE pointer to n_bytes bytes, any alignment                                                  */
    uint32_t n_bytes;     /* 1 .. 2^20                                                                                       */
    uint32_t format;      /* 1 + the slot of the format; 0: plain, no interleaver and no table                               */
    uint32_t branch0;     /* 0 .. B-1: the branch of out[0]                                                                  */
    uint32_t flags;       /* PSK_SOFT_FRAME_INVERT                                                                           */
    uint32_t pad[2];      /* zero                                                                                            */
} psk_soft_frame_cut_in_t;  /* 48 bytes */

typedef struct psk_soft_frame_cut {      /* one per frame of the LAST cut call */
    uint32_t flags;                      /*   0  PSK_SOFT_FRAME_DATA or _PLANNED, | the frame's flags shifted left by one   */
    uint32_t n_bytes;                    /*   4                                                                             */
    uint32_t span;                       /*   8                                                                             */
    uint32_t n_ones;                     /*  12                                                                             */
    uint32_t pad[4];                     /*  16  zero                                                                       */
} psk_soft_frame_cut_t;                  /* 32 bytes */

/* The word of slot `slot` (0 .. PSK_SOFT_FRAME_SLOTS - 1); a stream names it as word = slot + 1.  Redefining a slot waits for
 * the handle's last search launch first.  A control-plane-only handle records the word.
 * PSK_SOFT_ERR_INVALID_ARG: a null handle, a slot out of range, length outside 1 .. 64, bits of word or care at `length` and
 * above, care == 0. */
psk_soft_status psk_soft_frame_word_define(psk_soft_handle_t *h, uint32_t slot, uint32_t length, uint64_t word, uint64_t care);
/* The streams in[0 .. nstream-1], nstream = 1 .. PSK_SOFT_FRAME_MAX_STREAMS.  The bits must be complete on `stream` (a viterbi
 * call enqueued there just before is); with PSK_SOFT_OPT_DEFERRED_JOIN pending the call joins the side streams into `stream`
 * first, as the viterbi and rs entries do.  Two launches (fold, join); the call returns without waiting.  Every call replaces the
 * records.  A stream with word == 0 or bits == NULL is skipped: it gets the all-zero record.
 * Refusals (PSK_SOFT_ERR_INVALID_ARG before anything is enqueued or any record changes): a null pointer, nstream out of range; on
 * a stream that is not skipped a slot out of range or never defined, 2 max_diff >= C, a period above 2^20, n_bits outside
 * 1 .. 2^31, flag bits, a non-zero pad.
 * A control-plane-only handle checks the arguments, then leaves records with flags = PSK_SOFT_FRAME_PLANNED, length and n_windows,
 * everything else zero. */
psk_soft_status psk_soft_frame_search_device(psk_soft_handle_t *h, uint32_t nstream, const psk_soft_frame_search_in_t *in /* [nstream] */,
                                             void *stream);
/* waits like psk_soft_get_rs does and copies the records of the streams [first, first + n) of the last search call out.
 * PSK_SOFT_ERR_INVALID_ARG: a null pointer, n == 0, a range beyond the last call's nstream, no call yet. */
psk_soft_status psk_soft_get_frame_search(psk_soft_handle_t *h, uint32_t first, uint32_t n, psk_soft_frame_search_t *rec /* [n] */);
/* host only, pure: the definition for one stream on the host.  `in` is read as the entry reads it, with a HOST pointer in bits;
 * `word` is not looked at beyond being non-zero.  *rec is byte for byte what the device writes.  A skipped stream gives the zero
 * record.  Refuses what the entry and the word's define refuse of their arguments. */
psk_soft_status psk_soft_frame_search_host(uint32_t length, uint64_t word, uint64_t care, const psk_soft_frame_search_in_t *in,
                                           psk_soft_frame_search_t *rec);
/* the phases a workgroup of the fold folds (the kernel's constant; a tile of windows with period 0 is 256 times that) */
uint32_t psk_soft_frame_tile(void);

/* The format of slot `slot` (0 .. PSK_SOFT_FRAME_SLOTS - 1) and its table (256 bytes copied into memory the handle owns; NULL:
 * the identity); a frame names it as format = slot + 1.  Redefining a slot waits for the handle's last cut launch first.  A
 * control-plane-only handle records the format.
 * PSK_SOFT_ERR_INVALID_ARG: a null handle, a slot out of range, branches outside 1 .. 255, cell above 255,
 * branches (branches - 1) cell above 2^24. */
psk_soft_status psk_soft_frame_format_define(psk_soft_handle_t *h, uint32_t slot, uint32_t branches, uint32_t cell, const uint8_t *table);
/* The frames in[0 .. nframe-1], nframe = 1 .. PSK_SOFT_FRAME_MAX_FRAMES; stream, join and records as the search has them.  One
 * launch.  A frame with bits == NULL is skipped: it gets the all-zero record and nothing is written.
 * Refusals (PSK_SOFT_ERR_INVALID_ARG before anything is enqueued or any record changes): a null pointer, nframe out of range; on
 * a frame that is not skipped a format slot out of range or never defined, branch0 >= B, n_bytes outside 1 .. 2^20, unknown flag
 * bits, a non-zero pad, a null `out`.
 * A control-plane-only handle checks the arguments, then leaves records with n_bytes, span and flags = PSK_SOFT_FRAME_PLANNED |
 * the frame's flags shifted left by one, everything else zero. */
psk_soft_status psk_soft_frame_cut_device(psk_soft_handle_t *h, uint32_t nframe, const psk_soft_frame_cut_in_t *in /* [nframe] */,
                                          void *stream);
/* as psk_soft_get_frame_search, for the frames of the last cut call */
psk_soft_status psk_soft_get_frame_cut(psk_soft_handle_t *h, uint32_t first, uint32_t n, psk_soft_frame_cut_t *rec /* [n] */);
/* host only, pure: the definition for one frame on the host, with HOST pointers in bits and out; `format` is not looked at.  The
 * bytes at out and *rec are byte for byte what the device writes.  A skipped frame gives the zero record.  `table` NULL: the
 * identity. */
psk_soft_status psk_soft_frame_cut_host(uint32_t branches, uint32_t cell, const uint8_t *table, const psk_soft_frame_cut_in_t *in,
                                        psk_soft_frame_cut_t *rec);
/* host only, pure: the stream bytes from `bit` that a frame of n_bytes bytes touches, 1 + its greatest source index; 0 for
 * arguments the define or the entry refuses */
uint64_t psk_soft_frame_span(uint32_t branches, uint32_t cell, uint32_t branch0, uint32_t n_bytes);
uint64_t psk_soft_frame_search_bytes(void);     /* sizeof(psk_soft_frame_search_t), for bindings */
uint64_t psk_soft_frame_search_in_bytes(void);  /* sizeof(psk_soft_frame_search_in_t), for bindings */
uint64_t psk_soft_frame_cut_bytes(void);        /* sizeof(psk_soft_frame_cut_t), for bindings */
uint64_t psk_soft_frame_cut_in_bytes(void);     /* sizeof(psk_soft_frame_cut_in_t), for bindings */

#endif
