/* psk_soft_rs.h -- the psk_soft_rs_ family of the C ABI of libpsk_soft_hip.so: Reed-Solomon decoding of byte frames on the GPU.
 * Part of psk_soft_hip.h, which includes it inside its extern "C" block and behind the types it needs (psk_soft_handle_t,
 * psk_soft_status); include psk_soft_hip.h, not this file.  The ABI version is psk_soft_hip.h's and stays 2. */
#ifndef PSK_SOFT_RS_H
#define PSK_SOFT_RS_H
#ifndef PSK_SOFT_HIP_H
#error "include psk_soft_hip.h, which includes psk_soft_rs.h"
#endif

/* ---- frames as corrected bytes: Reed-Solomon decoding of byte frames (psk_soft_rs_device) ----------------------------------------
 * The K = 7 171/133 code is the inner code of the concatenated schemes (CCSDS telemetry, DVB-S) whose outer code is Reed-Solomon
 * over GF(256).  This call decodes frames of bytes that are already in device memory -- as psk_soft_viterbi_device writes them
 * with PSK_SOFT_VITERBI_PACKED -- with an RS code the caller defines, and writes the corrected bytes where the caller wants them;
 * it leaves one small record per frame.  Everything is GF(256) arithmetic, so the host definition (psk_soft_rs_host) and the
 * device agree to the byte.
 *
 * The call touches no demodulator state, statistics or history, and no other record.  Frames, codes and masks are read, never
 * written.
 *
 * Field.  GF(256) = GF(2)[x] / gfpoly; gfpoly is 0x100 .. 0x1ff and primitive: alpha = 2 has order 255.  Refused otherwise.
 * Code.  fcr = 0 .. 254; prim = 1 .. 254 with gcd(prim, 255) = 1; nroots = 2 .. 64; n = nroots + 1 .. 255, k = n - nroots;
 *   t = floor(nroots / 2).  Byte i of a codeword (i = 0 is first in memory) is the coefficient of x^(n-1-i); a shortened code is a
 *   full code with 255 - n zero bytes in front.  c is a codeword iff c(alpha^(prim (fcr + m))) = 0 for m = 0 .. nroots - 1.  These
 *   are the usual (symsize 8, gfpoly, fcr, prim, nroots, pad) parameters: CCSDS (255,223) is 0x187, 112, 11, 32; DVB (204,188) is
 *   0x11d, 0, 1, 16 with n = 204.
 * Interleave depth I = 1 .. 8.  A frame is n I bytes; codeword j (0 .. I-1) has its byte i at frame offset i I + j.
 * Mask (derandomiser), optional: mask_len = 0 .. n I bytes; frame byte q < mask_len is XORed with mask[q] as it is read.
 *   "Received" below means the bytes after the mask is applied.
 * Decoding.  For codeword j: if a codeword lies within t differing bytes of the received word, it is unique; the result is that
 *   codeword and n_err[j] is the number of differing bytes (0 .. t).  Otherwise the result is the received word unchanged and
 *   n_err[j] = PSK_SOFT_RS_FAILED.  A locator with a root in the pad of a shortened code is a failure, not a correction.  This is
 *   a definition by outcome and fixes no algorithm.
 * Output.  out[i I + j] is the result byte i of codeword j, for i < k; with the frame flag PSK_SOFT_RS_WITH_PARITY for i < n.
 *   Exactly k I (or n I) bytes are written and no byte outside them.
 * Pointers.  `in` and `out` may have any byte alignment (frames abut).  The kernel may read an aligned dword that holds a frame
 *   byte, nothing further.  Inputs are never written.  The outputs of a call may overlap neither each other nor any input: that
 *   is the caller's duty and is not checked.  In-place decoding is not supported.
 * Record.  One psk_soft_rs_t per frame of the LAST call, in the order of `in`; the entries j >= I are zero.  There are no
 *   per-frame totals: a binding sums.
 * Cost.  One frame never uses more than one wave of 64 lanes: only a call of thousands of frames fills the machine. */
#define PSK_SOFT_RS_SLOTS       16
#define PSK_SOFT_RS_MAX_FRAMES  (1u << 20)
#define PSK_SOFT_RS_MAX_DEPTH   8
#define PSK_SOFT_RS_MAX_ROOTS   64
#define PSK_SOFT_RS_FAILED      255
enum { PSK_SOFT_RS_WITH_PARITY = 1 };  /* psk_soft_rs_in_t.flags */
/* psk_soft_rs_t.flags: DATA or PLANNED, ORed with the frame's flags shifted left by one */
enum { PSK_SOFT_RS_DATA = 1, PSK_SOFT_RS_REC_WITH_PARITY = 2, PSK_SOFT_RS_PLANNED = 128 };

typedef struct psk_soft_rs_in {
    const uint8_t *in;    /* DEVICE pointer to the frame's first byte, any alignment; NULL: the frame is skipped             */
    uint8_t *out;         /* DEVICE pointer to the output: k I bytes, or n I with WITH_PARITY; any alignment                 */
    uint32_t code;        /* 1 + the slot of the code; 0: the frame is skipped                                               */
    uint32_t flags;       /* PSK_SOFT_RS_WITH_PARITY                                                                         */
    uint32_t pad[2];      /* zero                                                                                            */
} psk_soft_rs_in_t;       /* 32 bytes */

typedef struct psk_soft_rs {             /* one per frame of the LAST psk_soft_rs_device call */
    uint32_t flags;                      /* PSK_SOFT_RS_DATA or _PLANNED, | the frame's flags shifted left by one           */
    uint16_t n, k;
    uint8_t depth, nroots;
    uint8_t pad0[6];                     /* zero                                                                            */
    uint8_t n_err[8];                    /* per codeword: the bytes corrected (0 .. t), or PSK_SOFT_RS_FAILED               */
    uint16_t n_bit[8];                   /* per codeword: the bits that differ between received and result over all n bytes;
                                            0 when failed                                                                   */
    uint8_t pad1[24];                    /* zero                                                                            */
} psk_soft_rs_t;                         /* 64 bytes */

/* The code of slot `slot` (0 .. PSK_SOFT_RS_SLOTS - 1) and its mask (mask_len bytes; `mask` may be NULL when mask_len is 0),
 * copied into memory the handle owns; a frame names it as code = slot + 1.  Redefining a slot waits for the handle's last rs
 * launch first.  A control-plane-only handle records the code.
 * PSK_SOFT_ERR_INVALID_ARG: a null handle, a slot out of range, a gfpoly, fcr, prim, nroots, n or depth the text above refuses,
 * mask_len above n depth, a null mask with mask_len > 0. */
psk_soft_status psk_soft_rs_define(psk_soft_handle_t *h, uint32_t slot, uint32_t gfpoly, uint32_t fcr, uint32_t prim, uint32_t nroots,
                                   uint32_t n, uint32_t depth, const uint8_t *mask, uint32_t mask_len);
/* The frames in[0 .. nframe-1], nframe = 1 .. PSK_SOFT_RS_MAX_FRAMES.  The bytes must be complete on `stream` (a viterbi call
 * enqueued there just before is); with PSK_SOFT_OPT_DEFERRED_JOIN pending the call joins the side streams into `stream` first,
 * as the sync, demap and viterbi entries do.  One launch; the call returns without waiting.  Every call replaces the records.
 * A frame with code == 0 or in == NULL is skipped: it gets the all-zero record and nothing is written.
 * Refusals (PSK_SOFT_ERR_INVALID_ARG before anything is enqueued or any record changes): a null pointer, nframe out of range; on
 * a frame that is not skipped a slot out of range or never defined, unknown flag bits, a non-zero pad, a null `out`.
 * A control-plane-only handle checks the arguments, then leaves records with n, k, depth, nroots and flags =
 * PSK_SOFT_RS_PLANNED | the frame's flags shifted left by one, everything else zero. */
psk_soft_status psk_soft_rs_device(psk_soft_handle_t *h, uint32_t nframe, const psk_soft_rs_in_t *in /* [nframe] */, void *stream);
/* waits like psk_soft_get_viterbi does and copies the records of the frames [first, first + n) of the last call out.
 * PSK_SOFT_ERR_INVALID_ARG: a null pointer, n == 0, a range beyond the last call's nframe, no call yet. */
psk_soft_status psk_soft_get_rs(psk_soft_handle_t *h, uint32_t first, uint32_t n, psk_soft_rs_t *rec /* [n] */);
/* host only, pure: the definition for one frame on the host.  `in` is read as the entry reads it, with HOST pointers in in and
 * out; `code` is not looked at beyond being non-zero.  The bytes at out and *rec are byte for byte what the device writes
 * (flags = PSK_SOFT_RS_DATA | ...).  A skipped frame gives the zero record.  Refuses what the entry and psk_soft_rs_define refuse
 * of their arguments. */
psk_soft_status psk_soft_rs_host(uint32_t gfpoly, uint32_t fcr, uint32_t prim, uint32_t nroots, uint32_t n, uint32_t depth,
                                 const uint8_t *mask, uint32_t mask_len, const psk_soft_rs_in_t *in, psk_soft_rs_t *rec);
/* host only, pure: the systematic encoder.  Per codeword j the parity is the remainder of d(x) x^nroots by g(x) = prod over m of
 * (x - alpha^(prim (fcr + m))); data[i depth + j] is data byte i of codeword j (k depth bytes); the n depth bytes at frame_out are
 * the interleaved codewords with the mask applied. */
psk_soft_status psk_soft_rs_encode_host(uint32_t gfpoly, uint32_t fcr, uint32_t prim, uint32_t nroots, uint32_t n, uint32_t depth,
                                        const uint8_t *mask, uint32_t mask_len, const uint8_t *data /* [k depth] */,
                                        uint8_t *frame_out /* [n depth] */);
uint64_t psk_soft_rs_bytes(void);           /* sizeof(psk_soft_rs_t), for bindings */
uint64_t psk_soft_rs_in_bytes(void);        /* sizeof(psk_soft_rs_in_t), for bindings */

#endif
