/*
 * zkwg.h -- C-ABI of the MI355X-native batched witness generator ("zkwg") for the
 * zk-email `EmailVerifier` circom circuit.
 *
 * This is the drop-in boundary: a plain C interface (pointers
 * and sizes only, no torch / HIP types) that a host binding (N-API addon, ctypes,
 * cgo ...) calls in place of the circom-generated WASM witness calculator.
 *
 * What each entry point replaces in the reference (paths relative to the reference
 * repository root):
 *
 *   zkwg_circuit_create      <- `wasm_tester(circuit.circom, {...})`
 *                                packages/circuits/tests/email-verifier.test.ts:21-31
 *                                (compiling `component main = EmailVerifier(...)`,
 *                                tests/test-circuits/email-verifier-test.circom:5,
 *                                rsa-test.circom:5, sha-test.circom:5) and the
 *                                `${circuitName}.wasm` argument of
 *                                packages/helpers/src/chunked-zkey.ts:80-84
 *   zkwg_calculate_batch     <- `circuit.calculateWitness(input)`
 *                                packages/circuits/tests/email-verifier.test.ts:43
 *                                and the first half of `snarkjs.groth16.fullProve`
 *                                (packages/helpers/src/chunked-zkey.ts:80), batched
 *   zkwg_calculate_batch_device  same, inputs/outputs already resident in HBM
 *   zkwg_pack_input          <- the `CircuitInput` object built by
 *                                packages/helpers/src/input-generators.ts:190-252
 *   zkwg_wtns_size / zkwg_write_wtns <- `snarkjs wtns calculate` / generate_witness.js
 *                                docs/zk-email-docs/UsageGuide/README.md:132-140
 *   zkwg_write_sym           <- the compiler's `.sym` file used by
 *                                circom_tester `assertOut` (email-verifier.test.ts:204)
 *   per-email status codes   <- circom_runtime exception codes; 4 = "Assert Failed"
 *                                (email-verifier.test.ts:73-79)
 *
 * All witness values are integers mod the BN254 scalar prime r
 * (packages/helpers/src/constants.ts:1), stored as 32-byte little-endian,
 * non-Montgomery field elements exactly as in a `.wtns` data section.
 *
 * Threading: the circuit description of a handle is immutable after creation.  The handle also
 * owns launch bookkeeping (timing event rings, the removeSoftLineBreaks merge-chain slots, the
 * host-path staging buffers); the device entry points take an internal lock around it and select
 * the handle's device themselves (the caller's current HIP device is restored on return), so a
 * handle may be shared by threads that launch on different streams.  Ordering between a
 * zkwg_prepare_device and the zkwg_expand_device that reads its scratch buffer is the caller's
 * (same stream, or an event).  zkwg_calculate_batch (host buffers) runs one call at a time per
 * handle.  No global state except zkwg_last_error (thread-local).
 */
#ifndef ZKWG_H
#define ZKWG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 3): ZKWG_IN_NFIELDS = 13 (the record's former padding word is ZKWG_IN_RANGE_FLAGS: hand-built records must
 * zero it, a non-zero word fails the email); zkwg_expand_device accepts out_stride >= 32 W (multiple of 16);
 * zkwg_scratch_bytes includes the Montgomery-copy area (and, round 5, 612 bytes per 16-byte body chunk of staging for the
 * removeSoftLineBreaks chunk hashes, behind the image arrays); zkwg_segment.pad is kernel-private.
 * Added since without breaking 2: zkwg_expand_host / zkwg_set_host_expand, zkwg_circuit_attach_r1cs / zkwg_expand_abc_device /
 * zkwg_expand_abc_host / zkwg_abc_bytes, ZKWG_MAIN_FP_MUL, ZKWG_MAIN_REVEAL_SUBSTRING, ZKWG_MAIN_COUNT_SUBSTRING,
 * ZKWG_MAIN_EMAIL_REVEAL with zkwg_app_config / zkwg_circuit_create_app and the record fields ZKWG_IN_SUBSTRING_START /
 * ZKWG_IN_SUBSTRING_LEN (ZKWG_IN_NFIELDS = 15; they take no room in the records of the other mains), ZKWG_MAIN_CLEAN_EMAIL_ADDRESS. */
#define ZKWG_ABI_VERSION 3

/* `component main = ...` choices (the reference's own test mains). */
enum zkwg_main_kind {
  ZKWG_MAIN_EMAIL_VERIFIER = 0, /* EmailVerifier(maxHeader,maxBody,n,k,ignoreBodyHashCheck,0,0,0), public [pubkey] */
  ZKWG_MAIN_SHA256_BYTES = 1,   /* Sha256Bytes(maxHeader), public [paddedIn, paddedInLength] (sha-test.circom) */
  ZKWG_MAIN_RSA_VERIFIER = 2,   /* RSAVerifier65537(n,k), public [modulus] (rsa-test.circom) */
  ZKWG_MAIN_FP_MUL = 3,         /* FpMul(n,k), n*k <= 62, 2 <= k <= 17: inputs a, b, p in the pubkey / signature / message slots of the
                                   record (fp-mul-test.circom: FpMul(2,4); tests/fp-mul.test.ts:34-46) */
  ZKWG_MAIN_REVEAL_SUBSTRING = 4, /* RevealSubstring(maxLength, maxSubstringLength, shouldCheckUniqueness), no public inputs
                                   (helpers/reveal-substring.circom:13-50, reveal-substring-test.circom:5: (256, 16, 1)).
                                   max_header = maxLength, max_body = maxSubstringLength, n = shouldCheckUniqueness (0 / 1), k = 0, every
                                   flag 0; 2 <= max_body < max_header <= 65536, neither needs to be a multiple of 64 (the record pads).
                                   in[] in ZKWG_IN_HEADER, substringStartIndex in ZKWG_IN_BODY_HASH_INDEX, substringLength in ZKWG_IN_BODY_LEN */
  ZKWG_MAIN_COUNT_SUBSTRING = 5,/* CountSubstringOccurrences(maxLen, maxSubstringLen) (utils/array.circom:226-254,
                                   count-substring-occurrences-test.circom:5: (1024, 128)).  max_header = maxLen, max_body =
                                   maxSubstringLen, n = k = 0; 2 <= max_body <= max_header <= 65536.  in[] in ZKWG_IN_HEADER, substring[] in
                                   ZKWG_IN_BODY.  Both mains: elements are bytes; no `.sym` layout, no Montgomery-form output (BAD_CONFIG) */
  ZKWG_MAIN_EMAIL_REVEAL = 6,   /* EmailReveal(maxHeader, maxBody, n, k, ignoreBodyHashCheck, revealFromBody, maxSubstringLength,
                                   shouldCheckUniqueness, withNullifier), no public inputs (zk-email-verify_amd/circuits/email-reveal.circom):
                                   EmailVerifier + RevealSubstring over the header or the body + PackBytes of the revealed bytes +
                                   EmailNullifier(signature).  Created with zkwg_circuit_create_app only */
  ZKWG_MAIN_CLEAN_EMAIL_ADDRESS = 7 /* CleanEmailAddress(maxLength), no public inputs, output isValid (utils/email.circom:16-140,
                                   clean-email-address-test.circom:5: (32)).  max_header = max_body = maxLength, a multiple of 8 with
                                   8 <= maxLength <= 1024 (every chunk of PoseidonModular(2 maxLength) is a Poseidon(16)); n = k = 0, every
                                   flag 0.  encoded[] in ZKWG_IN_HEADER, decoded[] in ZKWG_IN_BODY (the record pads both slots); elements are
                                   bytes.  The template asserts nothing: every byte input has a witness (status 4 only for a record whose
                                   range flags are set).  No `.sym` layout, no attached constraint system, no Montgomery-form output
                                   (BAD_CONFIG) */
};

/* Witness layouts.  KEPT_V1 is the compact layout documented in DESIGN.md; SYM is KEPT_V1 re-ordered
 * (and thinned) to the witness indices of a circom `.sym` file, see zkwg_circuit_create_sym. */
enum zkwg_layout { ZKWG_LAYOUT_KEPT_V1 = 0, ZKWG_LAYOUT_SYM = 1 };

typedef struct zkwg_config {
  uint32_t main_kind;                /* enum zkwg_main_kind */
  uint32_t max_header;               /* maxHeadersLength (multiple of 64); substring mains: maxLength / maxLen, any value up to 65536;
                                        ZKWG_MAIN_CLEAN_EMAIL_ADDRESS: maxLength */
  uint32_t max_body;                 /* maxBodyLength   (multiple of 64; 0 if unused); substring mains: maxSubstringLength / maxSubstringLen;
                                        ZKWG_MAIN_CLEAN_EMAIL_ADDRESS: maxLength again */
  uint32_t n;                        /* bits per RSA limb   (121); ZKWG_MAIN_REVEAL_SUBSTRING: shouldCheckUniqueness (0 / 1) */
  uint32_t k;                        /* number of RSA limbs (17)  */
  uint32_t ignore_body_hash_check;   /* template flag, email-verifier.circom:42 */
  uint32_t enable_header_masking;    /* template flag: headerMask input, maskedHeader output */
  uint32_t enable_body_masking;      /* template flag: bodyMask input, maskedBody output */
  uint32_t remove_soft_line_breaks;  /* template flag: decodedEmailBodyIn input, RemoveSoftLineBreaks check */
  uint32_t layout;                   /* enum zkwg_layout */
} zkwg_config;

/* Fields of one packed input record (one record per email). */
enum zkwg_input_field {
  ZKWG_IN_HEADER = 0,         /* u8[max_header]  emailHeader / paddedIn / in (substring mains) / encoded (ZKWG_MAIN_CLEAN_EMAIL_ADDRESS) */
  ZKWG_IN_BODY = 1,           /* u8[max_body]    emailBody / substring (ZKWG_MAIN_COUNT_SUBSTRING) / decoded (ZKWG_MAIN_CLEAN_EMAIL_ADDRESS) */
  ZKWG_IN_PRECOMPUTED_SHA = 2,/* u8[32]          precomputedSHA                    */
  ZKWG_IN_PUBKEY = 3,         /* 17 x 16-byte LE limbs: pubkey / modulus           */
  ZKWG_IN_SIGNATURE = 4,      /* 17 x 16-byte LE limbs                             */
  ZKWG_IN_MESSAGE = 5,        /* 17 x 16-byte LE limbs (RSA main only)             */
  ZKWG_IN_HEADER_LEN = 6,     /* u32 emailHeaderLength / paddedInLength            */
  ZKWG_IN_BODY_LEN = 7,       /* u32 emailBodyLength / substringLength (ZKWG_MAIN_REVEAL_SUBSTRING) */
  ZKWG_IN_BODY_HASH_INDEX = 8,/* u32 bodyHashIndex / substringStartIndex (ZKWG_MAIN_REVEAL_SUBSTRING) */
  ZKWG_IN_HEADER_MASK = 9,    /* u8[max_header]  headerMask (enable_header_masking)  */
  ZKWG_IN_BODY_MASK = 10,     /* u8[max_body]    bodyMask   (enable_body_masking)    */
  ZKWG_IN_DECODED_BODY = 11,  /* u8[max_body]    decodedEmailBodyIn (remove_soft_line_breaks) */
  ZKWG_IN_RANGE_FLAGS = 12,   /* u32 bit f = an element of field f did not fit its packed slot (generic path)  */
  ZKWG_IN_SUBSTRING_START = 13, /* u32 substringStartIndex (ZKWG_MAIN_EMAIL_REVEAL; absent from the records of the other mains) */
  ZKWG_IN_SUBSTRING_LEN = 14,   /* u32 substringLength     (ZKWG_MAIN_EMAIL_REVEAL) */
  ZKWG_IN_NFIELDS = 15
};

/* Per-email status: circom_runtime exception codes. */
enum zkwg_status {
  ZKWG_OK = 0,
  ZKWG_ERR_ASSERT_FAILED = 4, /* a `===` / assert failed: "Assert Failed" */
  ZKWG_ERR_WITNESS_NOT_REDUCED = 7 /* zkwg_prover_prove_witnesses: a witness value is not below the group order r (no circom_runtime
                                      code: those are 1 .. 6); such a witness gets no proof */
};

/* API return codes (negative = misuse / runtime failure). */
enum zkwg_rc {
  ZKWG_RC_OK = 0,
  ZKWG_RC_BAD_CONFIG = -1,
  ZKWG_RC_BAD_ARG = -2,
  ZKWG_RC_NO_DEVICE = -3,
  ZKWG_RC_HIP_ERROR = -4,
  ZKWG_RC_OOM = -5
};

typedef struct zkwg_circuit zkwg_circuit_t;

int zkwg_abi_version(void);
const char* zkwg_strerror(int rc_or_status);

/* Create / destroy.  `device` is a HIP device ordinal; device < 0 builds a
 * layout-only handle (no GPU needed: sizes, .sym, .wtns and packing still work,
 * zkwg_calculate_* return ZKWG_RC_NO_DEVICE). */
int zkwg_circuit_create(const zkwg_config* cfg, int device, zkwg_circuit_t** out);
/* Same, with the witness ordered as a compiled circuit's `.sym` file says (the file circom writes next
 * to the `.r1cs`/`.wasm`; circom_tester `loadSymbols`, packages/circuits/tests/email-verifier.test.ts:204,
 * and the order `groth16.prove(zkey, wtns)` needs, packages/helpers/src/chunked-zkey.ts:80).  `sym_text` =
 * the file's bytes: lines "labelIdx,witnessIdx,componentIdx,name", witnessIdx -1 = eliminated.  Every
 * signal the file keeps must be one this schedule produces (same qualified name); signals it eliminates
 * are dropped from the output.  `alias_text` (may be NULL): rename rules "ours=theirs", one per line,
 * applied to this library's names first (compiler-generated names of anonymous components).
 * On ZKWG_RC_BAD_CONFIG, zkwg_last_error() says which signal did not match.  cfg->layout is ignored. */
int zkwg_circuit_create_sym(const zkwg_config* cfg, int device, const char* sym_text, uint64_t sym_len,
                            const char* alias_text, uint64_t alias_len, zkwg_circuit_t** out);
/* Complete witnesses for a circuit compiled without full simplification (the reference documents
 * `circom ... --O0`, docs/zk-email-docs/UsageGuide/README.md:56-64): besides the `.sym` file the compiler's
 * `.r1cs` is given.  Every signal the file numbers beyond the ones this library's schedule produces (aliases,
 * constants, linear combinations -- 2.4 M of the 3.1 M signals of EmailVerifier(576,192) at O0) is derived from
 * the LINEAR constraints of the `.r1cs` (triangular elimination at creation).  On the device the file's witness is
 * written in ONE pass from the compact image (csrc/zkwg_o0.h): every wire has an 8-byte descriptor (the bit / byte /
 * image word it copies, or the result of a row), the rows that are real sums are evaluated into extensions of the
 * image by the row kernels at the end of zkwg_prepare_device, and zk_expand3_o0 streams all wires out -- no staging
 * buffer, no gather, launches of one handle need no ordering beyond prepare-before-expand of the same scratch buffer,
 * and Montgomery-form output works (zkwg_expand_montgomery_device).  Rates: DESIGN.md section 16.  Creation fails
 * with zkwg_last_error naming the first signal that is neither produced nor linearly defined (a quadratic
 * signal of a template this schedule does not implement, e.g. zk-regex's real BodyHashRegex).  Multi-
 * dimensional signal names (`a[t][k]`) are accepted by both `.sym` entry points. */
int zkwg_circuit_create_full(const zkwg_config* cfg, int device, const char* sym_text, uint64_t sym_len,
                             const char* alias_text, uint64_t alias_len, const uint8_t* r1cs, uint64_t r1cs_len,
                             zkwg_circuit_t** out);
uint64_t zkwg_linear_rows(const zkwg_circuit_t* c);                       /* derived signals of such a handle */
/* `.sym` layouts: out[s] = witness index of the default (kept-v1) layout's slot s, 0xffffffff if the file
 * eliminated it; returns the number of kept-v1 slots (0 for a handle without a `.sym`). */
uint64_t zkwg_layout_map(const zkwg_circuit_t* c, uint32_t* out, uint64_t cap);
/* BodyHashRegex from the template text.  EmailVerifier takes its regex circuit from the generated file
 * `@zk-email/zk-regex-circom/circuits/common/body_hash_regex.circom` (packages/circuits/email-verifier.circom:5,
 * 126-127), which is not part of the reference tree.  zkwg_circuit_create builds zkwg's own DFA circuit for that
 * regex; this entry builds the schedule FROM a supplied template instead: the file (and what it includes --
 * regex_helpers.circom, circomlib's comparators/gates/bitify; circomlib falls back to the restatement carried by
 * the library) is parsed and elaborated for msg_bytes = max_header, every hint / quadratic signal becomes a gate
 * evaluated on the device (kernel zk_net_eval), linear signals are substituted away.  Signal names follow the
 * compiler's (anonymous components `<T>_<line>_<offset>`), so a `.sym` (and `.r1cs`, see
 * zkwg_circuit_create_full) of the same circuit can be passed along; both may be NULL for the compact layout.
 * Supported subset and limits: zk-email-verify_amd/csrc/zkwg_circom.h. */
typedef struct zkwg_regex_source {
  const char* circom_path;    /* the generated template file                                              */
  const char* include_dirs;   /* ':'-separated directories searched for include "..." (may be NULL)       */
  const char* template_name;  /* NULL: "BodyHashRegex"; instantiated as template_name(max_header)(header) */
} zkwg_regex_source;
int zkwg_circuit_create_regex(const zkwg_config* cfg, int device, const zkwg_regex_source* regex,
                              const char* sym_text, uint64_t sym_len, const char* alias_text, uint64_t alias_len,
                              const uint8_t* r1cs, uint64_t r1cs_len, zkwg_circuit_t** out);
/* Application main (ZKWG_MAIN_EMAIL_REVEAL): `cfg` as for EmailVerifier (n = 121, k = 17, max_header / max_body by its rules, every
 * masking / soft-line-break flag 0), `app` what sits on top of it.  Public signals, all outputs: pubkeyHash, (with_nullifier)
 * emailNullifier = Poseidon(1)(PoseidonLarge(121, 17)(signature)), revealed[ceil(max_substring / 31)] = the revealed bytes packed
 * little-endian, 31 per field element (utils/bytes.circom:28-60).  Inputs: EmailVerifier's, then substringStartIndex
 * (ZKWG_IN_SUBSTRING_START) and substringLength (ZKWG_IN_SUBSTRING_LEN), set with zkwg_pack_field or written as u32 at
 * zkwg_input_offset.  Status 4 on anything EmailVerifier or RevealSubstring asserts and on a range flag (a source element that
 * is not a byte, a start or length above 2^32 - 1).  Bounds: 2 <= max_substring < the source's maximum length;
 * reveal_from_body = 1 needs the body-hash check; each flag 0 or 1.  No `.sym` / numbered layout, no attached constraint system,
 * no Montgomery-form output, no regex template (BAD_CONFIG): proofs go through zkwg_prover_create_wtns.  zkwg_circuit_create
 * refuses kind 6 with BAD_CONFIG (zkwg_last_error names this call). */
typedef struct zkwg_app_config {
  uint32_t reveal_from_body;   /* 0: RevealSubstring over emailHeader, 1: over emailBody */
  uint32_t max_substring;      /* maxSubstringLength */
  uint32_t check_uniqueness;   /* shouldCheckUniqueness: the match matrix of CountSubstringOccurrences is part of the circuit */
  uint32_t with_nullifier;     /* the emailNullifier output and its two Poseidon instances */
} zkwg_app_config;
int zkwg_circuit_create_app(const zkwg_config* cfg, const zkwg_app_config* app, int device, zkwg_circuit_t** out);
/* out[0..8): kept signals, temporaries, gates, assertion gates, chunks, 64-gate steps, LDS words that hold gate
 * values, gates on the evaluator's 64-bit path (handles created by zkwg_circuit_create_regex) */
int zkwg_regex_info(const zkwg_circuit_t* c, uint64_t out[8]);
int zkwg_linear_complete_host(const zkwg_circuit_t* c, uint8_t* witness); /* layout-only handles: host evaluation */
/* layout-only handles of a fully numbered circuit: the linear plan (copies + rows over the kept-v1 witness) on the host --
 * `out` (32 * zkwg_witness_len bytes) from one compact kept-v1 witness (the default layout of the same configuration) */
int zkwg_o0_gather_host(const zkwg_circuit_t* c, const uint8_t* kept_witness, uint8_t* out);
const char* zkwg_last_error(void);   /* detail of the calling thread's last ZKWG_RC_BAD_CONFIG */
void zkwg_circuit_destroy(zkwg_circuit_t* c);

/* Geometry. */
uint64_t zkwg_witness_len(const zkwg_circuit_t* c);   /* W: field elements per witness */
uint64_t zkwg_witness_bytes(const zkwg_circuit_t* c); /* 32 * W */
uint32_t zkwg_num_public(const zkwg_circuit_t* c);    /* outputs + public inputs: w[1..nPublic] */
uint64_t zkwg_input_stride(const zkwg_circuit_t* c);  /* bytes per packed input record */
uint64_t zkwg_input_offset(const zkwg_circuit_t* c, int field); /* byte offset inside a record */
uint64_t zkwg_scratch_bytes(const zkwg_circuit_t* c, uint64_t n_emails); /* device scratch for a batch */
/* The same without the Montgomery-copy area, which lies at the end of the buffer: enough for every entry point except the ones that
 * produce Montgomery-form values from this buffer (zkwg_expand_montgomery_device, zkwg_expand_abc_device with montgomery = 1) -- those
 * need zkwg_scratch_bytes.  For removeSoftLineBreaks = 1 the image is mostly field elements and this is half the size. */
uint64_t zkwg_scratch_bytes_standard(const zkwg_circuit_t* c, uint64_t n_emails);

/* Pack one email's inputs into a record (host helper; every pointer may be NULL
 * when the main kind does not use that field).  Limbs are 17 x 16-byte LE. */
int zkwg_pack_input(const zkwg_circuit_t* c, uint8_t* record,
                    const uint8_t* header, uint32_t header_len,
                    const uint8_t* body, uint32_t body_len,
                    const uint8_t* precomputed_sha, const uint8_t* pubkey_limbs,
                    const uint8_t* signature_limbs, const uint8_t* message_limbs,
                    uint32_t body_hash_index);
/* Generic input path: `CircuitInput` values are arbitrary field elements
 * (packages/helpers/src/input-generators.ts:6-18; circom_runtime normalises each one mod r and
 * stores it as a full 32-byte element), while the packed record keeps bytes / u32 / 128-bit limbs.
 * zkwg_pack_field takes `count` elements of input field `field` (ZKWG_IN_*) as 32-byte
 * little-endian integers (any 256-bit value; reduced mod r here), starting at element `first` of
 * that field, and writes them into the record.  An element that does not fit its slot keeps its
 * low bits and sets bit `field` of the record's ZKWG_IN_RANGE_FLAGS word: the kernels then fail the
 * email exactly where the circuit's own range check of that signal fails -- Num2Bits(8) of
 * lib/sha.circom:27,60,70, Num2Bits(log2Ceil(max)) of email-verifier.circom:58,116, Num2Bits(n) of
 * lib/rsa.circom:28,118,123, AssertBit of utils/bytes.circom:151-154, the RLC equality of
 * helpers/remove-soft-line-breaks.circom:124 -- status 4, "Assert Failed".  Call after
 * zkwg_pack_input (which clears the flags). */
int zkwg_pack_field(const zkwg_circuit_t* c, uint8_t* record, int field, uint64_t first,
                    const uint8_t* values32, uint64_t count);
/* headerMask / bodyMask of one record (flag variants; either pointer may be NULL). */
int zkwg_pack_masks(const zkwg_circuit_t* c, uint8_t* record, const uint8_t* header_mask, const uint8_t* body_mask);
/* decodedEmailBodyIn of one record (remove_soft_line_breaks = 1): max_body bytes, the output of
 * `removeSoftLineBreaks(bodyRemaining)` (packages/helpers/src/input-generators.ts:127-158, 241-244). */
int zkwg_pack_decoded_body(const zkwg_circuit_t* c, uint8_t* record, const uint8_t* decoded_body);

/* Host-buffer batch: H2D of `packed_inputs` (n_emails records), kernels, D2H of
 * n_emails witnesses (32*W bytes each, `out_stride` bytes apart; out_wtns may be
 * NULL to fetch only `status`).  Processes the batch in tiles of `max_tile` emails
 * (0 = 256, reduced if HBM is short); witness buffers are double-buffered so the
 * D2H copy of tile t overlaps the kernels of tile t+1.  One call at a time per handle. */
int zkwg_calculate_batch(zkwg_circuit_t* c, const uint8_t* packed_inputs, uint64_t n_emails,
                         uint8_t* out_wtns, uint64_t out_stride, int32_t* status,
                         uint64_t max_tile);

/* Batched input generation on the device (the step right before the path): restates
 * generateEmailVerifierInputsFromDKIMResult (packages/helpers/src/input-generators.ts:190-252) with
 * sha256Pad / generatePartialSHA (sha-utils.ts:30-111) and toCircomBigIntBytes (binary-format.ts:71-83).
 * All pointers are device pointers; `selector` is the optional shaPrecomputeSelector (shared by the
 * batch).  d_records receives n packed input records (zkwg_input_stride each); d_gen_status[i]:
 *   0 ok | 1 header does not fit maxHeadersLength | 2 remaining body longer than maxBodyLength
 *   | 3 selector not found in the body | 4 body longer than body_stride
 *   | 5 needle absent | 6 needle not unique | 7 needle empty or too long (zkwg_generate_reveal_inputs_device only, below).
 * EmailVerifier, and EmailReveal with its two index fields left zero for the caller. */
typedef struct zkwg_dkim_batch {
  const uint8_t* headers;        /* [n][header_stride] canonical signed header bytes */
  const uint32_t* header_len;    /* [n] */
  const uint8_t* bodies;         /* [n][body_stride] canonical body bytes (NULL if ignoreBodyHashCheck) */
  const uint32_t* body_len;      /* [n] */
  const uint8_t* body_hash_b64;  /* [n][44] bodyHash, base64 text */
  const uint8_t* pubkey_be;      /* [n][256] RSA modulus, big-endian */
  const uint8_t* signature_be;   /* [n][256] signature, big-endian */
  const uint8_t* selector;       /* shaPrecomputeSelector bytes or NULL */
  uint32_t header_stride, body_stride, selector_len;
} zkwg_dkim_batch;
int zkwg_generate_inputs_device(zkwg_circuit_t* c, const zkwg_dkim_batch* batch, uint64_t n_emails,
                                void* d_records, void* d_gen_status, void* hip_stream);

/* EmailReveal's records from one needle per email: what zkwg_generate_inputs_device writes, and
 * substringStartIndex / substringLength with it -- nothing of an email is looked at on the host.  Needle i is
 * bytes[first[i] .. first[i + 1]) (first has n_emails + 1 entries; both are device pointers, the shape of
 * zkwg_dkim_verify_args.keys / key_first).  The handle says where it is looked for:
 *   reveal_from_body = 0   first occurrence in the canonical signed header bytes [0, header_len); the body, if the circuit has one,
 *                          is prepared as zkwg_generate_inputs_device prepares it, shared selector included
 *   reveal_from_body = 1   first occurrence `pos` in the canonical body bytes [0, body_len), never in the SHA padding; the body's
 *                          SHA prefix is cut at (pos / 64) * 64: precomputedSHA is the state after those bytes, emailBody the padded
 *                          body from there on, substringStartIndex = pos - cut.  batch->selector_len must be 0.
 * A true substring search in both cases.  A needle that spans a "=\r\n" soft line break of the body is not found: the circuit reveals
 * the canonical bytes, not the decoded ones.  d_gen_status[i]: the codes of zkwg_generate_inputs_device, and
 *   5 the needle does not occur in the source | 6 the needle occurs more than once in the record's source array (max_header or
 *   max_body bytes, SHA padding and zero fill included, overlapping occurrences counted: what CountSubstringOccurrences counts) and
 *   the circuit checks uniqueness | 7 the needle is empty or longer than max_substring.
 * Order: 1, 3 and 4 as zkwg_generate_inputs_device reports them, then 7, 5, 2 (with the needle's cut), 6.  A record with a code has
 * a body length of 0 and both index fields 0.
 * ZKWG_RC_BAD_CONFIG: the handle is not ZKWG_MAIN_EMAIL_REVEAL; ZKWG_RC_BAD_ARG: a null pointer, or a selector with body needles.
 * One kernel on `hip_stream`: no allocation, no synchronisation. */
typedef struct zkwg_needles {
  const uint8_t* bytes;          /* the needles, one behind the other */
  const uint32_t* first;         /* [n_emails + 1] */
} zkwg_needles;
int zkwg_generate_reveal_inputs_device(zkwg_circuit_t* c, const zkwg_dkim_batch* batch, const zkwg_needles* needles,
                                       uint64_t n_emails, void* d_records, void* d_gen_status, void* hip_stream);

/* Device-resident batch below the boundary: for a host without a tensor library (the Node host of the
 * reference) that feeds a device-side consumer.  The records go to the device once; the compute kernels of sub-batch i + 1
 * (`prep` emails, default 1024) run on one internal stream while sub-batch i is expanded tile by tile (`tile` emails, default
 * 512) on another; witnesses are written into a ring of TWO tiles in HBM that is overwritten as the batch proceeds -- the
 * ring is placed where HBM takes the stores fastest (once per handle: the first tile's expansion is timed into spare
 * candidate buffers, zkwg_resident_placement reports the timings; ZKWG_PLACE_RING=0 disables).  After each tile's expansion
 * has been enqueued `consumer` (may be NULL) is called on the calling thread with the tile's device pointer, the distance
 * between consecutive witnesses, the index of its first email, its email count and the HIP stream the expansion was
 * enqueued on: work the consumer enqueues on that stream sees the complete tile and finishes before the ring slot is reused
 * (a GPU prover's entry point; packages/helpers/src/chunked-zkey.ts:80-84 is the call it completes).  What comes back to the
 * host: status[n] and, if `table` is given, n rows of 100 bytes {status i32, pubkeyHash, shaHi, shaLo} -- never the witnesses
 * (56.9 MB each: use zkwg_calculate_batch for that, PCIe-bound).  zkwg_calculate_batch_multi with out_wtns = NULL runs this
 * on every device. */
typedef void (*zkwg_tile_fn)(void* user, int device, const void* d_tile, uint64_t witness_stride, uint64_t first_email,
                             uint64_t count, void* hip_stream);
int zkwg_calculate_batch_resident(zkwg_circuit_t* c, const uint8_t* packed_inputs, uint64_t n_emails, int32_t* status,
                                  uint8_t* table, uint64_t tile, uint64_t prep, zkwg_tile_fn consumer, void* user);
int zkwg_resident_placement(const zkwg_circuit_t* c, float* ms, int cap, int kept[2]);
/* Give the buffers zkwg_calculate_batch_resident keeps in the handle (records, scratch, the two-tile witness ring, statuses) back to the
 * device; the next call allocates and places them again.  For a service that shares the GPU between circuits. */
int zkwg_resident_release(zkwg_circuit_t* c);


/* Host expansion (the delivered-to-host rate; the consumer is snarkjs on the host,
 * packages/helpers/src/chunked-zkey.ts:80-84).  A witness crosses PCIe at 32 bytes per signal (56.9 MB per email) although
 * its information is the 0.45 MB image the prepare kernels leave.  zkwg_expand_host runs the segment decoders of
 * zk_expand on the host (same source, csrc/zkwg_expand_dec.h) over an image that was copied to host memory:
 * `records` = the n packed input records, `scratch_host` = a host copy of the scratch buffer of
 * zkwg_prepare_device(c, ., n, ...) (zkwg_scratch_bytes(c, n) bytes; only the image arrays are read), emails
 * [first, first + count) go to `out` (16-byte aligned), written with non-temporal stores by `threads` host threads.
 * Not available for zkwg_circuit_create_full handles (their row results are computed on the device).
 * zkwg_set_host_expand(c, threads > 0) makes zkwg_calculate_batch use this route: per tile H2D records -> prepare
 * kernels -> D2H of the image, the host expanding tile t while the device prepares tile t + 1 (0 = device expansion + D2H
 * of the witnesses, the default).  Both routes give identical bytes. */
int zkwg_expand_host(const zkwg_circuit_t* c, const uint8_t* records, uint64_t n_emails, const uint8_t* scratch_host,
                     uint64_t first, uint64_t count, uint8_t* out, uint64_t out_stride, int threads);
int zkwg_set_host_expand(zkwg_circuit_t* c, int threads);

/* A HIP stream (returned as void*, NULL on failure) restricted to the compute units whose bit is set in `mask`
 * (`words` x 32 bits, CU i = bit i; hipExtStreamCreateWithCUMask).  Optional tuning aid: the prepare kernels are latency-bound
 * and few; confined to a few CUs they do not take wave slots from zk_expand on the others (bench.py --prep-cus). */
void* zkwg_stream_create_masked(int device, const uint32_t* mask, int words);
void zkwg_stream_destroy(void* stream);

/* Page-locked host memory for `out_wtns` (optional): with it the D2H copy of one tile overlaps the
 * kernels of the next tile. */
void* zkwg_alloc_pinned(uint64_t bytes);
void zkwg_free_pinned(void* p);

/* Device-resident batch: every pointer is a device pointer on the handle's
 * device; `hip_stream` is a hipStream_t passed as void* (NULL = default stream).
 * d_scratch must hold zkwg_scratch_bytes(c, n_emails).  Asynchronous. */
int zkwg_calculate_batch_device(zkwg_circuit_t* c, const void* d_packed_inputs, uint64_t n_emails,
                                void* d_out_wtns, uint64_t out_stride, void* d_status,
                                void* d_scratch, void* hip_stream);

/* The two phases of zkwg_calculate_batch_device, separately launchable (e.g. on different
 * streams, with different granularity):
 *   zkwg_prepare_device  runs every compute kernel for n_emails and leaves their compact
 *                        images in d_scratch (zkwg_scratch_bytes(c, n_emails)) + d_status;
 *   zkwg_expand_device   streams the witnesses of emails [first, first+count) of that prepared
 *                        batch into d_out_wtns (count * 32 W bytes) -- the HBM-write-bound kernel.
 * The images are ~1 % of the witness size, so a whole batch can be prepared at once while its
 * witnesses are expanded tile by tile into a smaller output ring.
 * remove_soft_line_breaks = 1: the serial Poseidon merge chain of a prepared batch runs on an internal
 * side stream (it is latency-bound and would stall the caller's stream for ~0.2 s); d_status and the
 * scratch images are complete once a zkwg_expand_device call on that scratch buffer has been ordered
 * (it waits for the chain), so keep at most 16 scratch buffers in flight per handle. */
int zkwg_prepare_device(zkwg_circuit_t* c, const void* d_packed_inputs, uint64_t n_emails, void* d_status,
                        void* d_scratch, void* hip_stream);
/* (out_stride: distance between consecutive witnesses in d_out_wtns, >= 32 * W and a multiple of 16) */
int zkwg_expand_device(zkwg_circuit_t* c, const void* d_packed_inputs, uint64_t n_emails, const void* d_scratch,
                       uint64_t first, uint64_t count, void* d_out_wtns, uint64_t out_stride, void* hip_stream);

/* Throttle for pipelined use: when zkwg_prepare_device runs concurrently with zkwg_expand_device of
 * the previous batch, cap the resident zk_rsa wavefronts per CU (each holds 164 VGPRs) so that the
 * HBM-bound expand kernel keeps its occupancy.  0 = no cap (default; lowest prepare latency). */
int zkwg_set_prepare_throttle(zkwg_circuit_t* c, int rsa_wavefronts_per_cu);
/* Measurement aid (tools/beside.py): zkwg_prepare_device launches only the kernels whose bit is
 * set -- bit 0 zk_sha_chain, 1 zk_sha_trace, 2 zk_net_eval, 3 zk_misc_ev, 4 zk_rsa, 5 zk_poseidon9*, 6 zk_rslb_chunks,
 * 7 zk_rslb_chain, 8 the row kernels of numbered / constraint-attached handles, 9 zk_app_tail (zk_substr shares bit 4, zk_cea_chunks
 * bit 6, zk_cea_tail bit 7).  Default 0xffffffff (everything); with a
 * partial mask the images of the batch are NOT complete, so only timing may be taken from such a call. */
int zkwg_set_prepare_mask(zkwg_circuit_t* c, uint32_t kernel_mask);

/* Time the dominant kernel(s) of the last zkwg_calculate_batch_device call with
 * HIP events recorded on the launch stream.  Returns ms in *ms for kernel index
 * `which` (see zkwg_kernel_name); negative rc if timing was not enabled. */
int zkwg_set_timing(zkwg_circuit_t* c, int enable);
int zkwg_last_kernel_ms(zkwg_circuit_t* c, int which, float* ms);
/* Sum of kernel `which`'s durations over the launches recorded since zkwg_set_timing(c, 1)
 * (at most the last 512 launches), and how many launches that sum covers. */
int zkwg_timing_summary(zkwg_circuit_t* c, int which, float* total_ms, uint32_t* launches);
int zkwg_num_kernels(const zkwg_circuit_t* c);
const char* zkwg_kernel_name(const zkwg_circuit_t* c, int which);
/* Witness slots (field elements) written per email by kernel `which`. */
uint64_t zkwg_kernel_slots(const zkwg_circuit_t* c, int which);

/* `.wtns` container: 4-byte magic "wtns", u32 version 2,
 * u32 nSections 2; section 1: u32 n8=32, 32-byte LE prime, u32 nWitness;
 * section 2: nWitness x 32-byte LE values. */
uint64_t zkwg_wtns_size(const zkwg_circuit_t* c);
int zkwg_write_wtns(const zkwg_circuit_t* c, const uint8_t* witness, uint8_t* out, uint64_t out_cap);

/* Symbol table of the layout in force, one line per witness slot: "slot,slot,0,name\n"
 * (the `.sym` line format `labelIdx,varIdx,componentIdx,name`).  Returns bytes
 * needed; writes at most cap bytes. */
uint64_t zkwg_write_sym(const zkwg_circuit_t* c, char* out, uint64_t cap);

/* ---- `.r1cs` reader + constraint check on the device ----------------------------
 * Replaces circom_tester's `await circuit.checkConstraints(witness)`, which every circuit test of the
 * reference calls right after calculateWitness (packages/circuits/tests/email-verifier.test.ts:44,
 * sha.test.ts, rsa.test.ts, ...): for each constraint of the compiled circuit, (A.w)*(B.w) == C.w mod r.
 * `bytes` = the iden3 `.r1cs` file circom wrote (field must be BN254 Fr).  device < 0: parse only. */
typedef struct zkwg_r1cs zkwg_r1cs_t;
int zkwg_r1cs_load(const uint8_t* bytes, uint64_t len, int device, zkwg_r1cs_t** out);
void zkwg_r1cs_destroy(zkwg_r1cs_t* r);
/* out = {nWires, nPubOut, nPubIn, nPrvIn, mConstraints, nLabels} */
int zkwg_r1cs_info(const zkwg_r1cs_t* r, uint64_t out[6]);
/* n witnesses resident in HBM (32-byte LE values, `stride` bytes apart, stride >= 32*nWires):
 * d_first_bad[i] (u64) = index of the first violated constraint of witness i, UINT64_MAX if all hold.
 * A value >= r anywhere in a checked linear combination also counts as a violation. */
int zkwg_check_constraints_device(zkwg_r1cs_t* r, const void* d_witness, uint64_t n, uint64_t stride,
                                  void* d_first_bad, void* hip_stream);
/* Same for witnesses in host memory (staged through the device in tiles). */
int zkwg_check_constraints(zkwg_r1cs_t* r, const uint8_t* witness, uint64_t n, uint64_t stride, uint64_t* first_bad);
/* First stage of a Groth16 prover on the device-resident witness (what snarkjs' `groth16.prove` does first with the
 * witness: the evaluations A.w, B.w, C.w of every constraint; second half of `fullProve`,
 * packages/helpers/src/chunked-zkey.ts:80): d_abc[e] receives 3 * nConstraints field elements -- the A values, then
 * B, then C -- `abc_stride` (>= 96 * nConstraints) bytes apart.  A witness in Montgomery form
 * (zkwg_expand_montgomery_device; pass montgomery = 1) yields evaluations in Montgomery form, a standard-form witness
 * (montgomery = 0) standard-form ones; nothing is converted or copied to the host.  The flag only selects a shortcut
 * (a Montgomery-form 0 or 1 needs no product); the arithmetic is the same.  The transforms and the sums that follow are the prover
 * stages 2 and 3 below (zkwg_ntt_*, zkwg_msm_*); zkwg_prover_* runs all of them. */
int zkwg_r1cs_evaluate_device(zkwg_r1cs_t* r, const void* d_witness, uint64_t n, uint64_t stride, int montgomery,
                              void* d_abc, uint64_t abc_stride, void* hip_stream);

/* ---- prover hand-off -------------------------------------------------------------
 * The step after this path is `groth16.prove(zkey, wtns)` (second half of fullProve,
 * packages/helpers/src/chunked-zkey.ts:80).  A device-resident prover takes the witness where
 * zkwg_expand_device left it; this converts n_values 32-byte field elements in place between the
 * `.wtns` standard form and Montgomery form (x * 2^256 mod r), whichever its NTT / MSM kernels want. */
int zkwg_convert_montgomery_device(void* d_values, uint64_t n_values, int to_montgomery, void* hip_stream);
/* The fused form: zkwg_expand_device that writes every witness value directly as x * 2^256 mod r
 * (0 -> 0, 1 -> R, values below 2^16 from a table, the rest one Montgomery product) -- the witness
 * is still written exactly once and never read back, so handing it to a device prover costs no extra
 * HBM pass.  Same arguments and layout as zkwg_expand_device; bit-identical to zkwg_expand_device
 * followed by zkwg_convert_montgomery_device(.., 1, ..).  Needs the default portion size. */
int zkwg_expand_montgomery_device(zkwg_circuit_t* c, const void* d_packed_inputs, uint64_t n_emails,
                                  const void* d_scratch, uint64_t first, uint64_t count, void* d_out_wtns,
                                  uint64_t out_stride, void* hip_stream);
/* ---- prover stage 2 (SURVEY.md 8f4 "next"): the transforms between A.w | B.w | C.w and the H multi-exponentiation ----------
 * snarkjs groth16_prove.js [EXT, pinned in yarn.lock:7767-7800; ffjavascript F1Field]: A = ifft(A.w), Aodd = A[i] * inc^i,
 * Aodd_T = fft(Aodd) (likewise B, C), P_T = Aodd_T * Bodd_T - Codd_T on the domain of 2^power >= nConstraints + nPublic + 1
 * points, inc = the primitive 2^(power+1)-th root w[power + 1] (w[28] = 5^((r-1)/2^28), w[i] = w[i+1]^2).  Everything is in
 * Montgomery form (x * 2^256 mod r), as zkwg_expand_abc_device(montgomery = 1) writes it and as an MSM wants it.
 * zkwg_ntt_create builds the twiddle and coset tables of one domain size (2 x 32 bytes x 2^log2_n on the device).
 * zkwg_h_evaluations_device: d_abc = n_emails records of A.w | B.w | C.w (n_constraints values each, abc_stride bytes apart,
 * e.g. straight from zkwg_expand_abc_device); d_work = zkwg_ntt_work_bytes(plan, n_emails) bytes of scratch; d_out receives
 * 2^log2_n values per email, out_stride bytes apart.  n_emails <= 21845 per call.  Arithmetic-bound (~12 Montgomery products
 * per element and transform), not HBM-bound: DESIGN.md section 22.
 * zkwg_ntt_transform_device: stand-alone in-place transforms of n_polys arrays (natural order in and out; inverse includes
 * 1 / n) -- ffjavascript's Fr.fft / Fr.ifft on Montgomery-form data. */
typedef struct zkwg_ntt zkwg_ntt_t;
int zkwg_ntt_create(int device, uint32_t log2_n, zkwg_ntt_t** out);
void zkwg_ntt_destroy(zkwg_ntt_t* plan);
uint64_t zkwg_ntt_domain(const zkwg_ntt_t* plan);
uint64_t zkwg_ntt_work_bytes(const zkwg_ntt_t* plan, uint64_t n_emails);
int zkwg_ntt_transform_device(zkwg_ntt_t* plan, void* d_data, uint64_t n_polys, int inverse, void* hip_stream);
int zkwg_h_evaluations_device(zkwg_ntt_t* plan, const void* d_abc, uint64_t abc_stride, uint64_t n_constraints, uint64_t n_emails,
                              void* d_work, void* d_out, uint64_t out_stride, void* hip_stream);

/* Device buffers mapped from physical chunks (HIP virtual-memory API; chunk_bytes = 0: 1 GiB): the allocator for the output ring of
 * zkwg_expand_device and any other large store target.  A buffer from hipMalloc may take zk_expand's stores 12-20 % slower than
 * another of the same size (round 4); a buffer mapped chunk by chunk does not (tools/chunkbench.hip, profiles/r05/r05_e_chunkbench.txt)
 * -- no spare candidates, no transient memory.  The pointer is an ordinary device pointer; free it with zkwg_device_free_chunked. */
int zkwg_device_alloc_chunked(int device, uint64_t bytes, uint64_t chunk_bytes, void** out);
/* the same with `extra` spare candidate chunks: every candidate takes a probe fill of zk_expand's store shape on a mapping of its own,
 * the fastest are kept and mapped back to back, the others released (transient: `extra` chunks).  rates[0 .. *n_rates): GB/s of the
 * candidates in creation order (rates may be NULL). */
int zkwg_device_alloc_chunked_ex(int device, uint64_t bytes, uint64_t chunk_bytes, uint32_t extra, void** out, float* rates, uint32_t cap,
                                 uint32_t* n_rates);
int zkwg_device_free_chunked(void* ptr);

/* ---- prover stage 3: the multi-exponentiations of groth16_prove.js (reference call site:
 * packages/helpers/src/chunked-zkey.ts:80-84, the second half of fullProve) -----------------------------------------------
 * pi_a, pib1, pi_c and resH are  sum_i scalar_i * base_i  over BN254 G1 with the zkey's bases (affine, x | y in Montgomery form,
 * 64 bytes each, the point at infinity all zeros -- sections 5, 6, 8, 9 of the file), pi_b the same over G2 (section 7: x.c0 | x.c1 |
 * y.c0 | y.c1, 128 bytes), with the witness resp. the H evaluations of zkwg_h_evaluations_device as scalars (32 bytes each,
 * standard or Montgomery form).  zkwg_msm_create / _create_g2 upload the bases of one such sum (window_bits = 0: chosen from n);
 * zkwg_msm_create_device takes bases already in device memory (group 1 / 2; not owned).  zkwg_msm_g1_device / _g2_device compute
 * the sum for the n scalars at d_scalars, d_work = zkwg_msm_work_bytes bytes of scratch (256-byte aligned), and return the point as
 * the zkey would store it (affine, Montgomery form, 64 / 128 bytes; zeros = infinity).  ones_apart = 1 for witness scalars (mostly
 * 0 / 1: the bases with scalar 1 are summed by a plain reduction tree instead of all landing in one bucket).  Bucket method, signed
 * windows, XYZZ accumulators: DESIGN.md section 23.  Scalars must be CANONICAL (below the group order r; a Montgomery-form scalar is
 * reduced by its conversion): the signed windows cover 255 bits, a value of 2^255 or more would lose its top carry.
 * zkwg_fixed_base_device: d_out[i] = scalar_i * G for the group's generator (G1: (1, 2); G2: the EIP-197 generator) -- how a key
 * with a KNOWN trapdoor becomes bases (tests, tools/bench_prove.py; a real key comes from its .zkey). */
typedef struct zkwg_msm zkwg_msm_t;
int zkwg_msm_create(int device, const uint8_t* bases, uint64_t n, int window_bits, zkwg_msm_t** out);
int zkwg_msm_create_g2(int device, const uint8_t* bases, uint64_t n, int window_bits, zkwg_msm_t** out);
int zkwg_msm_create_device(int device, int group, const void* d_bases, uint64_t n, int window_bits, zkwg_msm_t** out);
void zkwg_msm_destroy(zkwg_msm_t* plan);
uint64_t zkwg_msm_work_bytes(const zkwg_msm_t* plan);
int zkwg_msm_window_bits(const zkwg_msm_t* plan);
int zkwg_msm_group(const zkwg_msm_t* plan);
int zkwg_msm_g1_device(zkwg_msm_t* plan, const void* d_scalars, int scalars_montgomery, int ones_apart, void* d_work, uint8_t* out_xy,
                       void* hip_stream);
int zkwg_msm_g2_device(zkwg_msm_t* plan, const void* d_scalars, int scalars_montgomery, int ones_apart, void* d_work, uint8_t* out_xy,
                       void* hip_stream);
/* asynchronous form: the sum is left at d_out_xyzz as an accumulator in XYZZ coordinates (Montgomery form; 128 bytes for a G1 plan,
 * 256 for a G2 plan) and nothing is synchronised -- the sums of several proofs can be in flight on several streams, which is what
 * hides the serial tail of each.  zkwg_msm_finish_host: n downloaded accumulators -> n points as the zkey stores them. */
int zkwg_msm_enqueue_device(zkwg_msm_t* plan, const void* d_scalars, int scalars_montgomery, int ones_apart, void* d_work, void* d_out_xyzz,
                            void* hip_stream);
int zkwg_msm_finish_host(int group, const uint8_t* xyzz, uint64_t n, uint8_t* out_points);
/* Round 6: emails are the parallel axis of the sums too.  One launch series sums n_emails scalar vectors (scalar_stride bytes apart,
 * a multiple of 32) against the plan's bases and leaves n_emails accumulators at d_out_xyzz (128 / 256 bytes each, consecutive); d_work:
 * zkwg_msm_work_bytes_batch(plan, n_emails) bytes.  zkwg_msm_create_ex: window_bits (0: from n), slice0 = bucket entries per lane at the
 * first slice level (0: 16; 64 for 2^20 full-size scalars), table_budget = bytes the plan may spend on its K shifted copies of the bases
 * (0: what is free minus 4 GiB; too small: the classic layout, K bucket sets and a Horner pass -- zkwg_msm_precomputed tells).
 * For witness scalars one classification pass serves several plans: zkwg_msm_classify_device writes, for up to three plans whose bases
 * cover the scalars [first[t], first[t] + n_t), the per-email index lists of the scalars that are 1 and of the others that are not 0
 * (bases at infinity left out) into d_lists[t] (zkwg_msm_lists_bytes(plan, n_emails) bytes, 256-byte aligned), and
 * zkwg_msm_enqueue_lists_device sums with them (d_work: n_emails * zkwg_msm_work_bytes(plan) bytes). */
int zkwg_msm_create_ex(int device, int group, const void* bases, int bases_on_device, uint64_t n, int window_bits, int slice0, uint64_t table_budget,
                       zkwg_msm_t** out);
uint64_t zkwg_msm_work_bytes_batch(const zkwg_msm_t* plan, uint64_t n_emails);
uint64_t zkwg_msm_lists_bytes(const zkwg_msm_t* plan, uint64_t n_emails);
uint64_t zkwg_msm_estimate_work_bytes(int group, uint64_t n, int window_bits, int slice0);   /* per email, before a plan exists */
uint64_t zkwg_msm_table_bytes(const zkwg_msm_t* plan);
int zkwg_msm_precomputed(const zkwg_msm_t* plan);
int zkwg_msm_enqueue_batch_device(zkwg_msm_t* plan, const void* d_scalars, uint64_t scalar_stride, uint64_t n_emails, int scalars_montgomery, int ones_apart,
                                  void* d_work, void* d_out_xyzz, void* hip_stream);
int zkwg_msm_classify_device(zkwg_msm_t* const* plans, const uint64_t* first, uint32_t n_plans, const void* d_scalars, uint64_t scalar_stride, uint64_t n_scalars,
                             uint64_t n_emails, int scalars_montgomery, int ones_apart, void* const* d_lists, void* hip_stream);
int zkwg_msm_enqueue_lists_device(zkwg_msm_t* plan, const void* d_scalars, uint64_t scalar_stride, uint64_t n_emails, int scalars_montgomery, const void* d_lists,
                                  int with_ones, void* d_work, void* d_out_xyzz, void* hip_stream);
int zkwg_fixed_base_device(int device, int group, const void* d_scalars, uint64_t n, void* d_out, void* hip_stream);
/* pi_a, pi_b, pi_c from the five sums of one proof and the key's alpha / beta / delta points (groth16_prove.js: pi_a = alpha1 + sum_a +
 * r delta1, pi_b = beta2 + sum_b2 + s delta2, pi_c = sum_c + sum_h + s pi_a + r (beta1 + sum_b1 + s delta1) - r s delta1).  Points in
 * as the zkey stores them (affine, Montgomery form); r, s = the blinding scalars (32 bytes, little-endian, below the group order);
 * points out in STANDARD form, little-endian x | y (G2: x.c0 | x.c1 | y.c0 | y.c1): the integers of snarkjs' proof.json.  Host
 * arithmetic (a dozen group operations).  ZKWG_RC_BAD_ARG for a point that is not on its curve. */
int zkwg_groth16_assemble(const uint8_t* sum_a, const uint8_t* sum_b1, const uint8_t* sum_b2, const uint8_t* sum_c, const uint8_t* sum_h,
                          const uint8_t* vk_alpha1, const uint8_t* vk_beta1, const uint8_t* vk_beta2, const uint8_t* vk_delta1,
                          const uint8_t* vk_delta2, const uint8_t* r32, const uint8_t* s32, uint8_t* pi_a, uint8_t* pi_b, uint8_t* pi_c);

/* ---- the prover as one call (reference: the second half of snarkjs.groth16.fullProve, packages/helpers/src/chunked-zkey.ts:80-84) ----
 * zkwg_prover_create plans everything a circuit's proofs need once: it attaches the constraint system `r1cs` (over the handle's
 * witness layout, WITH the nPublic + 1 rows snarkjs appends to A; n_rows = its constraint count; NULL if already attached) to `c`,
 * builds the transform plan of the key's domain and the five multi-exponentiation plans over the key's bases (host pointers to
 * sections 5-9 of the .zkey, or device pointers with bases_on_device = 1), and allocates the buffers of `slots` proofs in flight:
 * 1-3 contexts of E = zkwg_prover_emails_per_series emails each (round 6: every stage is one launch series for the E emails of a
 * context; the contexts roll, nothing depends on the number of hardware queues).  zkwg_prover_prove_prepared: proofs of emails indices[0 .. n_idx) of a batch prepared with
 * zkwg_prepare_device(c, d_in, n, ..., d_scratch); blinding = n_idx x (r | s), 32-byte little-endian scalars below the group order
 * (random per proof); out_proofs = n_idx x 256 bytes: pi_a (x | y) | pi_b (x.c0 | x.c1 | y.c0 | y.c1) | pi_c (x | y), standard-form
 * little-endian integers -- the numbers of snarkjs' proof.json.  zkwg_prover_prove_batch: the same from n packed input records on the
 * host (status[i] = circom_runtime code of email i; the proof bytes of a failed email are zero). */
typedef struct zkwg_prover zkwg_prover_t;
typedef struct zkwg_proving_key {
  uint64_t n_wires, n_public, log2_domain;
  const void *a, *b1, *b2, *c, *h;            /* bases: n_wires G1, n_wires G1, n_wires G2, n_wires - n_public - 1 G1, 2^log2_domain G1 */
  int bases_on_device;                        /* 0: host memory (uploaded here), 1: device memory (not owned) */
  uint8_t alpha1[64], beta1[64], beta2[128], delta1[64], delta2[128];   /* as the zkey's header stores them */
} zkwg_proving_key;
int zkwg_prover_create(zkwg_circuit_t* c, int device, const uint8_t* r1cs, uint64_t r1cs_len, uint64_t n_rows, const zkwg_proving_key* key,
                       uint32_t slots, zkwg_prover_t** out);
/* The prover from the zkey ALONE, as `groth16.prove(zkey, wtns)` / `fullProve(input, wasm, zkey)` take it (chunked-zkey.ts:80-84): the
 * rows of A and B (the nPublic + 1 public rows included) come from section 4 of the file, C.w = A.w o B.w as snarkjs' buildABC1 forms
 * it, the bases from sections 5-9; `zkey` is only read during the call.  The handle's witness layout must be the key's (nVars wires). */
int zkwg_prover_create_zkey(zkwg_circuit_t* c, int device, const uint8_t* zkey, uint64_t zkey_len, uint32_t slots, zkwg_prover_t** out);
void zkwg_prover_destroy(zkwg_prover_t* p);
uint32_t zkwg_prover_emails_per_series(const zkwg_prover_t* p);
uint32_t zkwg_prover_contexts(const zkwg_prover_t* p);
int zkwg_prover_prove_prepared(zkwg_prover_t* p, const void* d_in, uint64_t n, const void* d_scratch, const uint64_t* indices, uint64_t n_idx,
                               const uint8_t* blinding, uint8_t* out_proofs);
int zkwg_prover_prove_batch(zkwg_prover_t* p, const uint8_t* packed, uint64_t n, const uint8_t* blinding, int32_t* status, uint8_t* out_proofs);

/* ---- `groth16.prove(zkey, wtns)` for ANY BN254 groth16 key: the prover of witnesses (no circuit handle) --------------------------------
 * zkwg_prover_create_wtns takes the .zkey and nothing else: section 4 becomes a row table on the device (csrc/zkwg_zkey_core.h), the
 * bases of sections 5-9 the plans of the five sums, `slots` proofs are in flight through the same rolling contexts as above.  Refused
 * with ZKWG_RC_BAD_CONFIG: a file that is not a BN254 groth16 key or whose section sizes disagree with its header, a coefficient with
 * wire >= nVars, row >= domainSize, matrix > 1 or value >= r, a row of more than 2^20 terms, nVars >= 2^31, and B1 / B2 base sets whose
 * points at infinity sit at different wires (the two sums share one classification of the witness).
 * zkwg_prover_prove_witnesses: n witnesses in host memory, `stride` (>= 32 * zkwg_prover_witness_len) bytes apart, each nVars 32-byte
 * little-endian standard-form values -- section 2 of a `.wtns` file (zkwg_wtns_parse tells where it starts); blinding = n x (r | s);
 * out_proofs = n x 256 bytes in the form of zkwg_prover_prove_batch.  status[i] = 0, or ZKWG_ERR_WITNESS_NOT_REDUCED when a value of
 * witness i is >= r (found on the device over all nVars values; its proof bytes are zero, nothing of it reaches the sums).  A witness
 * that violates a constraint still gets a proof, as from snarkjs: the verifier rejects it.  The witnesses of a series are copied through
 * pinned staging on the series' own stream, so the copy of one series overlaps the sums of another.
 * zkwg_prover_prove_witnesses_device: the same for witnesses already in device memory (16-byte aligned, stride a multiple of 16).
 * A.w | B.w | C.w (C.w = A.w o B.w, snarkjs' buildABC1) come from zk_zkey_abc (csrc/zkwg_kernels_zkey.hip); zkwg_prover_abc_device runs
 * that stage alone: n records of 3 * zkwg_prover_rows values, Montgomery form, abc_stride (>= 96 * rows, multiple of 32) bytes apart.
 * The email entry points (zkwg_prover_prove_prepared / _batch) return ZKWG_RC_BAD_ARG on such a prover, and these on a handle prover.
 * zkwg_zkey_check: the checks of creation on the host alone (no device). */
int zkwg_prover_create_wtns(int device, const uint8_t* zkey, uint64_t zkey_len, uint32_t slots, zkwg_prover_t** out);
uint64_t zkwg_prover_witness_len(const zkwg_prover_t* p);   /* nVars of the key */
uint32_t zkwg_prover_num_public(const zkwg_prover_t* p);
uint64_t zkwg_prover_rows(const zkwg_prover_t* p);          /* rows of A (the nPublic + 1 public rows included) */
int zkwg_prover_prove_witnesses(zkwg_prover_t* p, const uint8_t* witnesses, uint64_t stride, uint64_t n, const uint8_t* blinding, int32_t* status,
                                uint8_t* out_proofs);
int zkwg_prover_prove_witnesses_device(zkwg_prover_t* p, const void* d_witnesses, uint64_t stride, uint64_t n, const uint8_t* blinding, int32_t* status,
                                       uint8_t* out_proofs);
int zkwg_prover_abc_device(zkwg_prover_t* p, const void* d_witnesses, uint64_t stride, uint64_t n, void* d_abc, uint64_t abc_stride, void* hip_stream);
/* `.wtns` (magic "wtns", version 2; section 1: n8 = 32, the prime r, nWitness; section 2: 32 * nWitness bytes; either order):
 * *values_offset = where section 2's values start.  ZKWG_RC_BAD_CONFIG for anything else. */
int zkwg_wtns_parse(const uint8_t* wtns, uint64_t len, uint64_t* n_witness, uint64_t* values_offset);
int zkwg_zkey_check(const uint8_t* zkey, uint64_t zkey_len, uint64_t* n_vars, uint32_t* n_public, uint64_t* n_rows);

/* The same prover stage without a 32-byte witness in between: the constraint system `r1cs` (its wires = the handle's
 * witness layout: built-in, `.sym`, or -- since ABI 3 -- a fully numbered handle of zkwg_circuit_create_full, whose system is
 * the compiler's own `.r1cs`, the file a zkey is keyed to: every wire of every combination is substituted by the kept-v1
 * signal(s) it derives from) is attached to the handle once -- BEFORE the
 * first zkwg_scratch_bytes / zkwg_prepare_device call that should serve it, the compact image grows by the results of the
 * combinations that are genuine sums, and only a prepare that follows the attachment writes the SHA-256 trace words the
 * descriptors name (an EmailVerifier handle without a system keeps round records alone, csrc/zkwg_sha_rounds.h): a batch
 * prepared before the attachment needs a fresh zkwg_prepare_device -- and zkwg_expand_abc_device then writes A.w | B.w | C.w (3 * nConstraints values,
 * `abc_stride` >= zkwg_abc_bytes apart) of emails [first, first + count) straight from the prepared image: a combination
 * that is one wire is written like that wire, sums of bits and small integers are 64-bit integer rows, only the rest is
 * arithmetic mod r.  Bit-identical to zkwg_r1cs_evaluate_device on the expanded witness (montgomery = 1: to that of the
 * Montgomery-form witness).  Replaces the head of snarkjs' groth16.prove (packages/helpers/src/chunked-zkey.ts:80). */
int zkwg_circuit_attach_r1cs(zkwg_circuit_t* c, const uint8_t* r1cs, uint64_t len);
uint64_t zkwg_abc_bytes(const zkwg_circuit_t* c);
int zkwg_expand_abc_device(zkwg_circuit_t* c, const void* d_packed_inputs, uint64_t n_emails, const void* d_scratch,
                           uint64_t first, uint64_t count, int montgomery, void* d_abc, uint64_t abc_stride, void* hip_stream);
/* The same values (standard form) written by the host from a host copy of the scratch buffer, like zkwg_expand_host for the
 * witness: rows_on_host = 0 -- the image was prepared by the device with the system already attached (only the image crosses
 * PCIe); rows_on_host = 1 -- the row tables are evaluated on the host too (scratch_host is written; the complete path of a
 * layout-only handle, used by the CPU tests).  out: 16-byte aligned, out_stride >= zkwg_abc_bytes.
 * (removeSoftLineBreaks handles: the row kernels follow the merge chain on its side stream, so the image is complete once that
 * stream's work is -- i.e. after any expansion call on the scratch buffer has been ordered, or a device synchronisation.) */
int zkwg_expand_abc_host(const zkwg_circuit_t* c, const uint8_t* packed_inputs, uint64_t n_emails, uint8_t* scratch_host,
                         uint64_t first, uint64_t count, int rows_on_host, uint8_t* out, uint64_t out_stride);
/* Layout-only handles of a fully numbered circuit (zkwg_circuit_create_full with device < 0): the complete witness of emails
 * [first, first + count) from a host copy of their images, evaluated through the same descriptor / row tables the device
 * kernels read (scratch_host is written: the row results).  A test hook like zkwg_o0_gather_host; device handles keep these
 * tables on the device only (BAD_CONFIG). */
int zkwg_expand_full_host(const zkwg_circuit_t* c, const uint8_t* packed_inputs, uint64_t n_emails, uint8_t* scratch_host,
                          uint64_t first, uint64_t count, uint8_t* out, uint64_t out_stride);

/* ---- the groth16 set-up: zKey.newZKey(r1cs, ptau) on the device (csrc/zkwg_setup_core.h) ----------------
 * The step between "compute the witness" and "prove" of the reference's workflow (docs/zk-email-docs/UsageGuide/README.md:145-180,
 * `snarkjs groth16 setup circuit.r1cs pot.ptau circuit.zkey`): a compiler-format .r1cs and a PREPARED powers-of-tau file give the
 * initial key (gamma = delta = 1, no contributions) as a .zkey that zkwg_prover_create_zkey / zkwg_prover_create_wtns and snarkjs'
 * provers read.  Section 10 is 64 zero bytes and a count of 0 (the circuit hash is not computed: `snarkjs zkey verify` refuses the
 * file, no prover looks there).  An unprepared file is prepared by zkwg_ptau_prepare (below); chunked keys and other curves are not
 * built; phase 2: below.
 *
 * zkwg_setup_slices: the points the set-up reads, in the zkey's form (affine, little-endian Montgomery words, zeros = infinity), for
 * the circuit's domain 2^power: [L_j(tau)]_1, [L_j(tau)]_2, [alpha L_j(tau)]_1, [beta L_j(tau)]_1 (2^power points each) and
 * [L_j(tau)]_1 of the domain 2^(power + 1).  Host pointers (on_device = 0) or device pointers (1).  zkwg_ptau_parse fills it with
 * pointers INTO the caller's buffer (an mmap: a power-21 file is 2 - 3 GB and is never copied); a caller may fill it by hand.
 * zkwg_ptau_parse checks the prime, the power and every section size before it reads a point.  A file without the Lagrange sections
 * 12 - 15 is refused ("Powers of tau is not prepared"), so is one whose power is below `power`.
 *
 * zkwg_zkey_new_size: the domain power the .r1cs needs (smallest p >= 1 with 2^p >= constraints + nPublic + 1) and the bytes of
 * its key.  zkwg_zkey_new writes the key to out_zkey (host memory, cap >= that size).  It is a one-shot call: it allocates its device
 * buffers, synchronises and frees them before it returns.  Refusals (ZKWG_RC_BAD_CONFIG, zkwg_last_error says which): whatever the
 * .r1cs reader refuses, nPublic + 1 >= nVars, slices of another power, a slice point that is not on its curve or not reduced (checked
 * on the device over every uploaded point), a wire with more than 2^27 terms in one sum. */
typedef struct zkwg_setup_slices {
  uint32_t power;
  uint32_t on_device;
  const void* tau_g1;         /* 2^power x 64 bytes */
  const void* tau_g2;         /* 2^power x 128 bytes */
  const void* alpha_tau_g1;   /* 2^power x 64 bytes */
  const void* beta_tau_g1;    /* 2^power x 64 bytes */
  const void* tau_g1_next;    /* 2^(power + 1) x 64 bytes */
  uint8_t alpha1[64], beta1[64], beta2[128];      /* the key's header points (always host memory) */
} zkwg_setup_slices;
int zkwg_ptau_parse(const uint8_t* ptau, uint64_t len, uint32_t power, zkwg_setup_slices* out);
int zkwg_zkey_new_size(const uint8_t* r1cs, uint64_t len, uint32_t* power, uint64_t* zkey_bytes);
int zkwg_zkey_new(int device, const uint8_t* r1cs, uint64_t len, const zkwg_setup_slices* slices, uint8_t* out_zkey, uint64_t cap,
                  uint64_t* out_len);
/* seconds and group operations of the last zkwg_zkey_new of this thread (tools/bench_setup.py):
 * {parse + plans, upload + curve check, sum A, sum B1, sum B2, sum K, H copy + download}, then per sum {additions, doublings} */
void zkwg_zkey_new_stats(double seconds[7], uint64_t ops[8]);

/* ---- phase 2: a contribution to a .zkey on the device (csrc/zkwg_phase2_core.h) -----------------------------
 * The reference's workflow requires "Phase 2" after the powers of tau (docs/zk-email-docs/UsageGuide/README.md:149,178-180; its next
 * command reads circuit_0001.zkey, the key AFTER a contribution): `snarkjs zkey contribute` / `zkey beacon`.  A contribution with
 * secret k sets delta1' = k delta1, delta2' = k delta2, C_i' = k^-1 C_i (section 8), H_j' = k^-1 H_j (section 9); sections 1, 3 - 7 and
 * alpha, beta, gamma are copied.  The record of section 10 (who contributed, the proof of knowledge of k) is the host layer's:
 * zkwg/phase2.py, and so is `zkey verify` (zkwg.phase2.verify: zkwg_zkey_new again, then zkwg_point_rlc_device with two arrays and
 * zkwg_pairing_check, below).  Not built: the circuit hash, chunked keys.
 *
 * zkwg_point_scale_device: d_out[i] = scalar * d_points[i] for n affine points in the zkey's form (64 / 128 bytes, little-endian
 * Montgomery words, zeros = infinity and stay zeros; group 1 / 2; device pointers, 16-byte aligned; d_out may be d_points).  scalar:
 * 32 bytes, little-endian, standard form, ANY value below 2^256 (not reduced modulo the group order: a G2 point outside the subgroup
 * is multiplied by the integer).  Every point is checked on its curve first; one that fails refuses the whole call: ZKWG_RC_BAD_CONFIG,
 * zkwg_last_error says "curve".  The call allocates 280 (G1) / 488 (G2) bytes per point for at most 2^20 points at a time, works on
 * hip_stream, synchronises it and frees its buffers before it returns.
 *
 * zkwg_zkey_apply_delta: the whole file operation, host memory in and out.  k: 32 bytes, little-endian, reduced modulo r by the call;
 * k = 0 mod r is refused, so are a file zkwg_zkey_check's header reader refuses (truncated, section sizes against the header), a
 * missing section 3, and a point of section 8, section 9 or delta that is not on its curve (ZKWG_RC_BAD_CONFIG + zkwg_last_error; the
 * bytes of `out` are unspecified then).  section10: the payload the new file gets as its section 10, verbatim.  out: cap >= what
 * zkwg_zkey_apply_delta_size gives for the same section10_len; the sections are written in the order 1 .. 10.  Sections 8 and 9 go
 * through the device in pieces of 2^20 points (294 MB of device memory), so a key of any domain fits. */
int zkwg_point_scale_device(int device, int group, const void* d_points, uint64_t n, const uint8_t* scalar, void* d_out, void* hip_stream);
int zkwg_zkey_apply_delta_size(const uint8_t* zkey, uint64_t len, uint64_t section10_len, uint64_t* out_bytes);
int zkwg_zkey_apply_delta(int device, const uint8_t* zkey, uint64_t len, const uint8_t* k, const uint8_t* section10, uint64_t section10_len,
                          uint8_t* out, uint64_t cap, uint64_t* out_len);
/* seconds and group operations of the last zkwg_zkey_apply_delta of this thread (tools/bench_phase2.py): {parse + copy of the unchanged
 * sections, upload + curve check, scaling of section 8, scaling of section 9, conversion + download}; {mixed additions, doublings} of
 * section 8, then of section 9 */
void zkwg_zkey_apply_delta_stats(double seconds[5], uint64_t ops[4]);

/* ---- prepare phase 2: the Lagrange sections of a powers-of-tau file on the device (csrc/zkwg_ptau_core.h) -------
 * `snarkjs powersoftau prepare phase2 pot.ptau pot_final.ptau`, the step between a ceremony file and zkwg_ptau_parse / zkwg_zkey_new
 * (docs/zk-email-docs/UsageGuide/README.md:145-180 names the prepared file).  powersoftau new / contribute / beacon: the next block; powersoftau verify: the one after.
 *
 * zkwg_group_ntt_device: the discrete Fourier transform of 2^log2_n affine points in the zkey's form (64 / 128 bytes, little-endian
 * Montgomery words, zeros = infinity; group 1 / 2; a device pointer, 16-byte aligned), IN PLACE, natural order in and out:
 *   inverse = 0:  out[j] = sum_k w^(jk) in[k]          inverse = 1:  out[j] = 2^-log2_n sum_k w^(-jk) in[k]
 * w: the 2^log2_n-th root of unity of zkwg_ntt_* (ffjavascript's Fr.w[log2_n]).  Points at infinity among the inputs, and equal or
 * opposite points meeting inside a butterfly, are computed, not excluded.  Every input point is checked first (words below q, on its
 * curve); one that fails refuses the whole call and leaves the points as they were: ZKWG_RC_BAD_CONFIG, zkwg_last_error says "curve".
 * There is NO subgroup check of G2 points (the set-up makes none either): points of the twist outside the subgroup of order r are
 * transformed as elements of the whole curve group only as far as w^k acts on them as an integer, which is not a transform.
 * The call allocates 312 (G1) / 520 (G2) bytes per point, works on hip_stream, synchronises it and frees its buffers before it
 * returns.  log2_n above 29 (G1: 168 GB) / 28 (G2: 140 GB) is refused with a message.
 *
 * zkwg_ptau_prepare: the file operation, host memory in and out (an mmap: only the prefixes the output needs are read).  power = 0:
 * the file's own power; 0 < power < the file's: the output is a file of that power (header power set, ceremonyPower kept, sections
 * 2 - 6 cut to 2 n - 1 | n | n | n | 1 points, n = 2^power, section 7 verbatim); above the file's: refused.  Output: sections 1 - 7,
 * then 12, 13, 14, 15 as zkwg_ptau_parse reads them: level q at point 2^q - 1, q = 0 .. power, section 12 one level more.  Level
 * q <= power is the inverse transform of the first 2^q points of section 2 / 3 / 4 / 5; level power + 1 of section 12 is the inverse
 * transform of the 2 n - 1 points of section 2 followed by ONE POINT AT INFINITY (tau^(2 n - 1) is not in a file of that power), also
 * when `power` cuts a larger file.  Refused (ZKWG_RC_BAD_CONFIG + zkwg_last_error): whatever the section walker refuses (sizes are
 * checked before any read), a file that has a section 12 - 15 ("already prepared"), a point of sections 2 - 5 that is not on its curve
 * or not reduced.  out: cap >= what zkwg_ptau_prepare_size gives for the same power.  Device memory: 376 bytes per point of the
 * largest level (2^(power + 1) G1 points; G2: 648 x 2^power) and 64 bytes per table entry (2^power). */
int zkwg_group_ntt_device(int device, int group, void* d_points, uint32_t log2_n, int inverse, void* hip_stream);
int zkwg_ptau_prepare_size(const uint8_t* ptau, uint64_t len, uint32_t power, uint64_t* out_bytes);
int zkwg_ptau_prepare(int device, const uint8_t* ptau, uint64_t len, uint32_t power, uint8_t* out, uint64_t cap, uint64_t* out_len);
/* seconds and group operations of the last zkwg_ptau_prepare of this thread (tools/bench_ptau.py): per section 12, 13, 14, 15
 * {upload + curve check, transforms up to the last stage's butterflies, last conversion + download} (12 values), then per section 32
 * values: the transform's seconds of level q at 12 + 32 * section + q; ops: per section {additions, doublings} */
void zkwg_ptau_prepare_stats(double seconds[140], uint64_t ops[8]);

/* ---- powers of tau: a contribution on the device (csrc/zkwg_ptau_key_core.h) --------------------------------
 * `snarkjs powersoftau contribute` / `beacon` on an UNPREPARED file, and the primitive underneath: many points, each times its own
 * scalar.  (`powersoftau new` needs no device: zkwg/ptau.py writes the generators.)  The record of section 7 -- who contributed, the
 * proofs of knowledge, the challenge chain -- is the host layer's (zkwg/ptau.py) and is ZKWG'S OWN: `snarkjs powersoftau verify` does
 * NOT accept the file; `prepare`, `setup` and every reader of the points do -- and `python -m zkwg.ptau verify` checks it (the next
 * block).  Not built: snarkjs-compatible challenge hashes, import / export challenge.
 *
 * zkwg_point_mul_device: d_out[i] = scalars[i] * d_points[i] for n affine points in the zkey's form (64 / 128 bytes, little-endian
 * Montgomery words, zeros = infinity and stay zeros; group 1 / 2; device pointers, 16-byte aligned; d_out may be d_points).
 * d_scalars: n x 32 bytes on the device, 16-byte aligned, little-endian, standard form, below r (a value at or above r is reduced
 * modulo r; 0 gives infinity).  zkwg_point_powers_device: the scalar of point i is c * t^(first + i) mod r, computed per lane on the
 * device from a table of t^(2^j) -- no scalar array crosses to the device.  c, t: 32 bytes, little-endian, reduced modulo r by the call;
 * either = 0 mod r is refused (ZKWG_RC_BAD_CONFIG), first + n must not pass 2^64 (ZKWG_RC_BAD_ARG).
 * Both: EVERY point is checked first (words below q, on its curve); one that fails refuses the whole call and leaves the points as they
 * were: ZKWG_RC_BAD_CONFIG, zkwg_last_error says "curve".  There is NO subgroup check of G2 points: a twist point outside the subgroup
 * of order r is multiplied by the integer scalars[i] (point_mul); the result of point_powers is unspecified for it.  The walk is a
 * regular signed window of 4 bits over a per-point table of 8 affine odd multiples in device memory: the calls allocate 2,024 (G1) /
 * 3,544 (G2) bytes per point for at most 2^20 (G1) / 2^19 (G2) points at a time, work on hip_stream, synchronise it and free their
 * buffers before they return.
 *
 * zkwg_ptau_apply_key: the file operation, host memory in and out.  Point k of sections 2 and 3 times tau^k (2 n - 1 G1 and n G2
 * points, n = 2^power), of section 4 times alpha tau^k, of section 5 times beta tau^k, the point of section 6 times beta
 * (zkwg_point_scale_device); section 1 is copied, section7 is the payload the new file gets as its section 7, verbatim.  The sections are
 * written in the order 1 .. 7.  tau, alpha, beta: 32 bytes, little-endian, reduced modulo r by the call.  Refused (ZKWG_RC_BAD_CONFIG +
 * zkwg_last_error; the bytes of `out` are unspecified then): whatever the section walker refuses (sizes are checked before any read), a
 * file that has a section 12 - 15 ("already prepared": its Lagrange sections would go stale), tau, alpha or beta = 0 mod r, a point of
 * sections 2 - 6 that is not on its curve or not reduced.  out: cap >= what zkwg_ptau_apply_key_size gives for the same section7_len. */
int zkwg_point_mul_device(int device, int group, const void* d_points, uint64_t n, const void* d_scalars, void* d_out, void* hip_stream);
int zkwg_point_powers_device(int device, int group, const void* d_points, uint64_t n, const uint8_t* c, const uint8_t* t, uint64_t first,
                             void* d_out, void* hip_stream);
int zkwg_ptau_apply_key_size(const uint8_t* ptau, uint64_t len, uint64_t section7_len, uint64_t* out_bytes);
int zkwg_ptau_apply_key(int device, const uint8_t* ptau, uint64_t len, const uint8_t* tau, const uint8_t* alpha, const uint8_t* beta,
                        const uint8_t* section7, uint64_t section7_len, uint8_t* out, uint64_t cap, uint64_t* out_len);
/* seconds and group operations of the last zkwg_ptau_apply_key of this thread (tools/bench_ptau_contribute.py): per section 2, 3, 4, 5
 * {upload + curve check, tables (odd multiples, made affine), walk, conversion + download} (16 values), [16] parse + copy of sections 1
 * and 7, [17] section 6; ops: per section {additions, doublings} */
void zkwg_ptau_apply_key_stats(double seconds[18], uint64_t ops[8]);

/* ---- powers of tau: verification (csrc/zkwg_verify_core.h, csrc/zkwg_pairing.h) -------------------------------------
 * What `python -m zkwg.ptau verify` (zkwg/ptau.py) is made of: the sections' millions of points are tested and folded on the device, the
 * few dozen pairings over the folded points run on the HOST, once.
 *
 * zkwg_pairing_check: is_one = (prod_i e(g1[i], g2[i]) == 1), BN254 optimal ate, one Miller loop per pair and ONE final exponentiation per
 * call.  Points in the zkey's form (64 / 128 bytes, Montgomery words, zeros = infinity: that pair contributes 1).  Refused with
 * ZKWG_RC_BAD_CONFIG + zkwg_last_error: a word >= q or a point off its curve ("curve"), a G2 point outside the subgroup of order r
 * ("subgroup": the criterion below, host build).  No device.
 *
 * zkwg_g2_subgroup_device: n affine G2 points in the zkey's form on the device (16-byte aligned).  *n_bad = how many are outside the
 * subgroup of order r, *first_bad = the lowest such index (unchanged when none).  Infinity counts as inside.  Every point is
 * curve-checked first as in zkwg_point_scale_device (one that fails refuses the call, "curve").  Criterion [EXT: El Housni, Guillevic,
 * Piellard]: with A = [u] Q, Q is in G2 iff A + Q + psi(A) + psi^2(A) = psi^3([2] A) -- 63 doublings instead of the 254 of [r] Q.
 * Pieces of at most 2^20 points (128 bytes of device memory a point); the call synchronises and frees what it allocated.
 *
 * zkwg_point_rlc_device: out_a = sum_i s_i A_i, out_b = sum_i s_i B_i over n points of one group (1 / 2); s_i: n x 16 bytes on the
 * device, little-endian (any 128-bit value).  d_b may be NULL (one sum; out_b is not written) and may overlap d_a -- d_b = d_a + one
 * point is the shifted form the powers checks need; d_b an array of its own (n points under the same scalars) is the form `zkey verify`
 * folds sections 8 / 9 of a key and of its initial key with.  Outputs: host memory, the zkey's form, zeros = infinity.  Curve check of every
 * point of both arrays first, refusal as above.  piece_points = 0: 2^22; every piece is one multi-exponentiation plan in the classic
 * layout, and the partial sums of the pieces are added on the host.  zkwg_point_rlc32_device: the same with 32-byte scalars, standard
 * form, BELOW r (the plans' rule). */
int zkwg_pairing_check(const uint8_t* g1, const uint8_t* g2, uint32_t n, int* is_one);
int zkwg_g2_subgroup_device(int device, const void* d_points, uint64_t n, uint64_t* n_bad, uint64_t* first_bad, void* hip_stream);
int zkwg_point_rlc_device(int device, int group, const void* d_a, const void* d_b, uint64_t n, const void* d_scalars, uint64_t piece_points,
                          uint8_t* out_a, uint8_t* out_b, void* hip_stream);
int zkwg_point_rlc32_device(int device, int group, const void* d_a, const void* d_b, uint64_t n, const void* d_scalars, uint64_t piece_points,
                            uint8_t* out_a, uint8_t* out_b, void* hip_stream);

/* ---- checking proofs: batched groth16 verification (csrc/zkwg_pair_core.h, csrc/zkwg_pair_host.h) ----------------------
 * `snarkjs groth16 verify` (reference: packages/helpers/src/chunked-zkey.ts:93-101) for MANY proofs of one key.  With random 128-bit
 * r_i the proofs of a batch are all valid, up to an error of about 2^-128 per batch, iff
 *     FE( prod_i f(r_i A_i, B_i) . f(-S0 alpha, beta) . f(-V, gamma) . f(-Cs, delta) ) = 1,
 *     S0 = sum r_i,  V = S0 IC_0 + sum_j (sum_i r_i x_ij) IC_j,  Cs = sum_i r_i C_i     (f: the Miller function, FE: the final exponentiation).
 * The device runs what grows with the batch -- one Miller loop per proof on a lane pair, the subgroup test of its B_i, the scalings
 * r_i A_i and r_i C_i, the product tree; the host adds three Miller loops and ONE final exponentiation per check.  When the batch
 * check fails the host bisects over the per-proof values (downloaded once, the same r_i): with k bad proofs among n at most
 * min(2 n - 1, 1 + 2 k ceil(log2 n)) checks.  A batch of mostly bad proofs is slow by design: zkwg_groth16_verify_each (below) is the call
 * for proofs that may be bad.
 *
 * zkwg_miller_device: f[i] = Miller value of (g1[i], g2[i]) up to a factor in Fq2 (the final exponentiation removes it: FE(f[i]) is the
 * reduced pairing); inside[i] = g2[i] in the subgroup of order r (f[i] means nothing when it is not).  Device pointers, the zkey's point form
 * (zeros = infinity -> f = 1, inside = 1), 16-byte aligned; f: n x 384 bytes, six Fq2 of w^0 .. w^5 (w^6 = 9 + i) as Montgomery words.
 * Every point is curve-checked first; one that fails refuses the call ("curve").  n <= 2^20.
 * zkwg_fq12_product_device: out (384 bytes, host memory) = the product of the f[i] with use[i] != 0 (d_use NULL: all of them; none: 1),
 * as a tree of launches; exact, so the result does not depend on the tree.
 *
 * zkwg_groth16_verify_batch: ok[i] = 1 iff proof i verifies.  proofs: n x 256 bytes in the form zkwg_prover_prove_* writes (standard-form
 * little-endian integers); publics: n x n_public x 32 bytes, little-endian standard form; rand16: n x 16 bytes, every entry non-zero (a
 * zero entry: ZKWG_RC_BAD_ARG), or NULL = drawn from the operating system inside the call.  device >= 0: Miller loops, subgroup tests
 * and the per-proof scalings on that device; device = -1: the same algorithm on the host alone (zkwg_pairing.h) -- the yardstick and
 * what a machine without a GPU runs.  n <= 2^20.  ok[i] = 0 without refusing the call: a public input >= r, a coordinate >= q, A, B or
 * C off its curve or all zeros (infinity: what the prover writes for a failed email), B outside the subgroup of order r -- outside it
 * the pairing is not bilinear and the batch equation means nothing (snarkjs does not test this; arkworks does when it deserialises).
 * The key is checked once per call (every point reduced, on its curve, not infinity; beta2, gamma2, delta2 in the subgroup); a bad key is
 * refused with ZKWG_RC_BAD_CONFIG + zkwg_last_error ("curve" / "subgroup"), never turned into verdicts.  n = 0 is ZKWG_RC_OK.
 * Device memory: 1,001 bytes per proof beside what zkwg_point_mul_device takes while it runs (2,024), freed before the call returns.
 * zkwg_groth16_verify_stats, of this thread's last call: seconds = {host checks + upload, scalings, Miller + subgroup, product +
 * download, host pairing of the batch check, bisection}; counts = {pairs sent to the device (or made on the host), host final
 * exponentiations, proofs excluded before the device, proofs found bad after that (subgroup flag or bisection)}. */
int zkwg_miller_device(int device, const void* d_g1, const void* d_g2, uint64_t n, void* d_f, uint8_t* d_inside, void* hip_stream);
int zkwg_fq12_product_device(int device, const void* d_f, const uint8_t* d_use, uint64_t n, uint8_t* out, void* hip_stream);
typedef struct zkwg_verification_key {
  uint32_t n_public;
  uint8_t alpha1[64], beta2[128], gamma2[128], delta2[128];   /* as a zkey's header stores them */
  const uint8_t* ic;                                          /* (n_public + 1) x 64 bytes, the same form */
} zkwg_verification_key;
int zkwg_groth16_verify_batch(int device, const zkwg_verification_key* vk, uint64_t n, const uint8_t* proofs,
                              const uint8_t* publics, const uint8_t* rand16, uint8_t* ok);
void zkwg_groth16_verify_stats(double seconds[6], uint64_t counts[4]);
/* Per-proof verdicts (csrc/zkwg_fexp_core.h, csrc/zkwg_fexp_host.h): the final exponentiation on the device, and a verifier whose work
 * does not depend on how many proofs are bad -- what a service that takes proofs from strangers calls.
 *
 * zkwg_final_exp_device: out[i] = FE(f[i]) = f[i]^((q^12 - 1) / r), EXACT (the value of the host's 2,790-bit square-and-multiply, not a
 * power of it; FE(0) = 0).  n x 384 bytes both ways, the form zkwg_miller_device writes; device pointers, 16-byte aligned; d_out may be
 * d_f.  n <= 2^20; n = 0 is ZKWG_RC_OK; device < 0: ZKWG_RC_NO_DEVICE.  Easy part with one Fq inversion per value, three powers by u over
 * its non-adjacent form with Granger-Scott squarings, the hard part by the chain of Devegili, Scott and Dahab: 22 launches with fixed
 * control flow, the value in device memory between them (2,688 bytes per value, freed before the call returns).
 *
 * zkwg_groth16_verify_each: ok[i] = 1 iff proof i verifies, each proof on its own:
 *     FE( f(A_i, B_i) . f(-vkx_i, gamma) . f(-C_i, delta) ) = e(alpha, beta)  and  B_i in the subgroup of order r,   vkx_i = IC_0 + sum_j x_ij IC_j.
 * Arguments, per-proof rejections (ok[i] = 0, the call goes on) and refusals of the key as zkwg_groth16_verify_batch, without rand16:
 * there is no randomness and no bisection.  device >= 0: the scalings x_ij IC_j (zkwg_point_mul_device), their sum made affine by the
 * complete point formulas (a public input 0, equal and opposite summands; vkx_i at infinity contributes f = 1), three Miller loops per
 * proof and the final exponentiation of their product on that device; the host makes e(alpha, beta) once per call, by the same final
 * exponentiation, and compares.  device = -1: the same algorithm on the host alone.  n <= 2^20; the call works in pieces of at most
 * 349,525 proofs (3 pairs each in one Miller launch; fewer when n_public x proofs would pass 2^20 scaled points).  Device memory per
 * proof of a piece: 5,187 + 96 n_public bytes beside what zkwg_miller_device (192 per pair) and zkwg_point_mul_device (2,024 per scaled
 * point) take while they run.
 * zkwg_groth16_verify_each_stats, of this thread's last call: seconds = {host checks + e(alpha, beta) + upload, vkx, Miller + subgroup,
 * final exponentiation, download + compare, 0}; counts = {pairs through the Miller loop (3 per proof that passed the host checks),
 * values exponentiated (those proofs + 1 for e(alpha, beta)), proofs excluded before the device, proofs found bad after that}. */
int zkwg_final_exp_device(int device, const void* d_f, uint64_t n, void* d_out, void* hip_stream);
int zkwg_groth16_verify_each(int device, const zkwg_verification_key* vk, uint64_t n, const uint8_t* proofs, const uint8_t* publics,
                             uint8_t* ok);
void zkwg_groth16_verify_each_stats(double seconds[6], uint64_t counts[4]);

/* ---- the compact image as a device-side interchange format --------------------------
 * zkwg_prepare_device leaves, per email, a compact IMAGE in the scratch buffer (~0.45 MB instead of the 57 MB
 * witness of EmailVerifier(1024,1536)): `bits` (u64 words of LSB-first bit groups), `small` (u32 values) and
 * `fr` (32-byte standard-form field elements).  Together with the email's packed input record and the circuit's
 * static SEGMENT TABLE it determines every witness slot: zk_expand is nothing but the evaluation of that table.
 * A device consumer that can evaluate the table itself (an MSM that treats bit / byte scalars specially, a
 * constraint checker ...) therefore never needs the 32-byte-per-signal witness in HBM.
 *
 * Scratch layout for a batch of n emails (all offsets in bytes, 256-byte aligned; zkwg_image_layout):
 *   hstates  u32[n][hstate_words]   SHA-256 chaining states (internal to the prepare kernels)
 *   bits     u64[n][bits_words]
 *   small    u32[n][small_words]
 *   fr       u8 [n][fr_elems][32]
 * Segment semantics (slot = witness index, r = r0 + (slot - first_slot), rec = the email's input record):
 *   see enum zkwg_segment_type; the per-type comments state how slot r derives from image / record.
 *   Inverses of small integers d (|d| <= zkwg_inverse_table_half) are d^-1 mod r (0 for d = 0).
 * The table follows the handle's layout (kept-v1 or a `.sym` order); ZKWG_SEG_HOLE only occurs for
 * zkwg_circuit_create_full handles (slots derived afterwards from the `.r1cs`). */
enum zkwg_segment_type {
  ZKWG_SEG_SMALL = 0,    /* small[src + r]                                                            */
  ZKWG_SEG_FR = 1,       /* fr[src + r]                                                               */
  ZKWG_SEG_BITS = 2,     /* groups of a bits in b words: bit (r % a) of bits[src + (r / a) * b ...]    */
  /* types 3-5 and the ZKWG_SEG_BITS segment (a = 33, b = 1) that follows them cover one Sha256compression; its 952 words at src
   * are the block's TRACE.  EmailVerifier handles: c = first word in `small` of the block's 200-word round record (W[0..63],
   * A[-4..63], E[-4..63]: csrc/zkwg_sha_rounds.h states how every group derives from it), which is what zk_expand decodes; the
   * trace words are written only by a prepare of a handle created with zkwg_circuit_create_full or with a constraint system
   * attached.  Sha256Bytes handles: c = 0, no record, the trace is always written. */
  ZKWG_SEG_SHA_SP = 3,   /* 162-slot periods over 5 words (32,32,32,32,34 bits): SigmaPlus instances  */
  ZKWG_SEG_SHA_T1 = 4,   /* 131-slot periods over 4 words (32,32,32,35): T1 instances                 */
  ZKWG_SEG_SHA_T2 = 5,   /* 161-slot periods over 5 words (32,32,32,32,33): T2 instances              */
  ZKWG_SEG_ISZ = 6,      /* IsZero pairs: d = (i32)small[src + r/2]; even r: d == 0, odd r: d^-1       */
  ZKWG_SEG_SEL = 7,      /* 256 x ItemAtIndex(a): idx = (i32)small[src], digest words small[b..b+8)    */
  ZKWG_SEG_IN8 = 8,      /* rec[src + r]                                                              */
  ZKWG_SEG_IN8BITS = 9,  /* bit (r & 7) of rec[src + r/8]                                             */
  ZKWG_SEG_LIMB = 10,    /* 16-byte LE limb rec[src + 16 r]                                           */
  ZKWG_SEG_LTBITS = 11,  /* bits of (i32)small[src] + 2^a - i, i = r / (a+1), bit r % (a+1)            */
  ZKWG_SEG_REGSEL = 12,  /* SelectRegexReveal comparators (see csrc/zkwg_sched.h)                      */
  ZKWG_SEG_VSHIFT = 13,  /* VarShiftLeft.tmp[j][i] = small[b + (i + (small[src] & (2^(j+1)-1))) % a]    */
  ZKWG_SEG_B64BITS = 14, /* 6 bits of the Base64 value of char small[src + r/6]                        */
  ZKWG_SEG_B64 = 15,     /* Base64Lookup internals of char small[src + r/68]                           */
  ZKWG_SEG_DFA = 16,     /* BodyHashRegex DFA circuit arrays (a = kind, b/c = parameters)              */
  ZKWG_SEG_IN8MASK = 17, /* rec[src + r] * rec[a + r]                                                  */
  ZKWG_SEG_RSLB = 18,    /* RemoveSoftLineBreaks byte-derived arrays over rec[src ..]                  */
  ZKWG_SEG_HOLE = 19,    /* not produced by the schedule (zkwg_circuit_create_full: derived later)     */
  ZKWG_SEG_NET = 20      /* loaded regex template: slot r = small[src + r] decoded: 31-bit signed integer, bit 31 = inverse of it */
};
typedef struct zkwg_segment {
  uint64_t slot;     /* first witness slot */
  uint32_t nslots;
  uint32_t type;     /* enum zkwg_segment_type */
  uint32_t src, a, b, c;
  uint32_t r0;       /* index of the first element inside the logical array */
  uint32_t pad;
} zkwg_segment;
typedef struct zkwg_image_layout_t {
  uint64_t hstate_words, bits_words, small_words, fr_elems;   /* per email */
  uint64_t off_hstates, off_bits, off_small, off_fr;          /* byte offsets in the scratch buffer of n emails */
  uint64_t total_bytes;                                       /* = zkwg_scratch_bytes(c, n) */
} zkwg_image_layout_t;
int zkwg_image_layout(const zkwg_circuit_t* c, uint64_t n_emails, zkwg_image_layout_t* out);
uint64_t zkwg_segment_table(const zkwg_circuit_t* c, zkwg_segment* out, uint64_t cap);   /* returns the segment count */
uint32_t zkwg_inverse_table_half(const zkwg_circuit_t* c);

/* ---- multi-GPU (BASELINE.json configs[3]) -------------------------------------------
 * Emails are independent: the batch is cut into n_dev contiguous shards (zkwg_shard_range), shard i runs on
 * devices[i] through its own handle and host thread, and its witnesses reach `out_wtns` over that GPU's own
 * PCIe link -- no data-path collective.  The only exchange is the 100-byte/email result table
 * {status i32 LE, pubkeyHash, shaHi, shaLo (32-byte LE each)} gathered on devices[0] over RCCL / xGMI
 * (ncclGroupStart + ncclSend / ncclRecv) and copied to `table` (n x 100 bytes, may be NULL; then RCCL is
 * not touched).  For the other mains the 96 bytes are w[1..3] of the witness.  librccl.so is opened with
 * dlopen, and only when n_dev > 1. */
typedef struct zkwg_multi zkwg_multi_t;
void zkwg_shard_range(uint64_t n_emails, int n_shards, int i, uint64_t* first, uint64_t* count);
int zkwg_multi_create(const zkwg_config* cfg, const int* devices, int n_dev, zkwg_multi_t** out);
void zkwg_multi_destroy(zkwg_multi_t* m);
int zkwg_multi_devices(const zkwg_multi_t* m);
zkwg_circuit_t* zkwg_multi_circuit(zkwg_multi_t* m, int i);   /* the handle of shard i (geometry, packing) */
int zkwg_calculate_batch_multi(zkwg_multi_t* m, const uint8_t* packed_inputs, uint64_t n_emails,
                               uint8_t* out_wtns, uint64_t out_stride, int32_t* status, uint8_t* table,
                               uint64_t max_tile);

/* ---- DKIM verification of raw emails -------------------------------------------------
 * The step before zkwg_generate_inputs_device: `verifyDKIMSignature` of the reference (packages/helpers/src/dkim/index.ts:36-97)
 * for a batch of raw messages.  The host parses each message and canonicalises its few hundred bytes of signed header
 * (zkwg_dkim_parse); the device canonicalises the bodies (zk_dkim_body), hashes bodies and headers (zk_dkim_hash) and checks
 * bh= and the RSA signature against every candidate key (zk_dkim_verify).  rsa-sha256 only, moduli of 1024 .. 2048 bits,
 * e = 65537.  No DNS: the caller brings the keys.
 * Per-email status (zkwg_strerror gives the reference's words; precedence as dkim-verifier.ts:245-335: body hash, key, signature): */
enum zkwg_dkim_status {
  ZKWG_DKIM_PASS = 0,
  ZKWG_DKIM_NOT_FOUND = 101,        /* "DKIM signature not found for domain" D (zkwg_dkim_parsed.d holds D) */
  ZKWG_DKIM_MULTIPLE_FROM = 102,    /* "Multiple From header in email and domain for verification not specified" */
  ZKWG_DKIM_NO_KEY = 103,           /* "no key" */
  ZKWG_DKIM_BODY_HASH = 104,        /* "body hash did not verify" */
  ZKWG_DKIM_BAD_SIGNATURE = 105,    /* "bad signature" */
  ZKWG_DKIM_UNSUPPORTED = 106,      /* algorithm other than rsa-sha256, no key of 1024 .. 2048 bits with e = 65537, malformed or missing
                                       tags (h, bh, b; l= with non-digits; b= longer than 256 bytes), canonical header longer than its slot */
  ZKWG_DKIM_BODY_DOES_NOT_FIT = 107 /* the canonical body is longer than body_stride */
};
typedef struct zkwg_dkim_parsed {
  int32_t status;                /* PASS, NOT_FOUND, MULTIPLE_FROM or UNSUPPORTED */
  uint32_t header_len;           /* canonical signed header bytes (also set when they did not fit header_cap) */
  uint64_t body_offset, body_len;/* the raw body inside the message */
  uint32_t header_canon, body_canon;   /* 0 relaxed, 1 simple */
  uint32_t has_l;
  uint64_t l;                    /* l=, when has_l */
  uint8_t bh[32];                /* bh= decoded */
  char bh_b64[48];               /* bh= as text (44 characters) */
  uint8_t signature[256];        /* b= decoded, big-endian, right-aligned */
  uint32_t signature_len;
  char d[256], s[256], a[64], c[64];   /* d= (NOT_FOUND: the domain that was looked for), s=, a=, c= as written */
  uint64_t body_bound;           /* zkwg_dkim_parse_batch only: no canonical form of the body is longer (body_len + its bare LFs + 2):
                                    the body_stride that always fits */
} zkwg_dkim_parsed;
/* One message: picks the signature of `domain` (NULL or "": of the single From address), writes its canonical signed header
 * (the fields of h= bottom-up, then the signature field with b= emptied) to header_out[0 .. header_cap) and fills *out.
 * Returns out->status.  Never reads outside raw[0 .. len).  header_out = NULL: the header is not written (header_cap still bounds it).
 * zkwg_dkim_parse_batch: the fields of n messages (no headers) on `threads` host threads (0 = the machine's, at most 16) -- what a
 * caller needs to look the keys up (s=, d=) before zkwg_dkim_verify_batch. */
int zkwg_dkim_parse(const uint8_t* raw, uint64_t len, const char* domain, uint8_t* header_out, uint32_t header_cap, zkwg_dkim_parsed* out);
int zkwg_dkim_parse_batch(uint64_t n, const uint8_t* const* emails, const uint64_t* email_len, const char* domain, int32_t threads,
                          zkwg_dkim_parsed* out);

typedef struct zkwg_dkim_key {
  uint8_t modulus_be[256];       /* big-endian, right-aligned */
  uint32_t bits;                 /* of the modulus as the record states it; above 2048 the key is unsupported */
  uint32_t exponent;
} zkwg_dkim_key;
#define ZKWG_DKIM_SKIP_BODY_HASH 1u
typedef struct zkwg_dkim_verify_args {
  int32_t device;                /* HIP device, or -1: the same cores on the host */
  int32_t threads;               /* host threads: for the parser and the packing of the bodies, and for everything with device = -1;
                                    0 = as many as the machine has, at most 16 */
  uint64_t n;
  const uint8_t* const* emails;  /* [n] raw messages */
  const uint64_t* email_len;     /* [n] */
  const char* domain;            /* or NULL */
  const zkwg_dkim_key* keys;     /* the candidate keys of email i: keys[key_first[i] .. key_first[i + 1]), tried in order */
  const uint32_t* key_first;     /* [n + 1] */
  uint32_t flags;                /* ZKWG_DKIM_SKIP_BODY_HASH */
  uint32_t header_stride, body_stride;
  /* results on the host; every pointer but status may be NULL */
  int32_t* status;               /* [n] enum zkwg_dkim_status */
  int32_t* key_index;            /* [n] index among the email's keys of the one that verified, else -1 */
  uint8_t* headers;              /* [n][header_stride]; bytes beyond a header's length are not written */
  uint32_t* header_len;          /* [n] */
  uint8_t* bodies;               /* [n][body_stride]; bytes beyond a body's length are not written */
  uint32_t* body_len;            /* [n] */
  uint8_t* body_digest;          /* [n][32] SHA-256 of the canonical body */
  uint8_t* header_digest;        /* [n][32] SHA-256 of the canonical signed header */
  zkwg_dkim_parsed* parsed;      /* [n] */
  /* device >= 0: when given, the filled batch stays on the device (pubkey_be = the key that verified, else the first candidate;
   * signature_be; body_hash_b64 = bh=), ready for zkwg_generate_inputs_device; release it with zkwg_dkim_batch_free */
  zkwg_dkim_batch* device_batch;
  double* seconds;               /* [6] parse, upload, zk_dkim_body, zk_dkim_hash, zk_dkim_verify, download */
} zkwg_dkim_verify_args;
int zkwg_dkim_verify_batch(const zkwg_dkim_verify_args* args);
int zkwg_dkim_batch_free(int device, zkwg_dkim_batch* batch);

#ifdef __cplusplus
}
#endif
#endif /* ZKWG_H */
