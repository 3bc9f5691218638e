/* krep_gpu.h — C-ABI of the MI355X-native literal-scan backend for krep.
 *
 * This header is the drop-in boundary.  Everything here is plain C (pointers + sizes, no C++ and
 * no torch types).  It sits exactly where krep's own algorithm functions sit: behind the uniform
 * operator signature `search_func_t` (reference krep.h:98-101), which search_chunk_thread()
 * (krep.c:1950) and search_string() (krep.c:2169) call, and which select_search_algorithm()
 * (krep.c:1771) returns.  The structs below are layout-identical to the reference's
 * (krep.h:49-60 match_position_t / match_result_t, krep.h:65-94 search_params_t) so a caller built
 * against krep.h can pass its own objects straight through.  If krep.h was included first its
 * definitions are used and ours are skipped.
 *
 * Error behaviour: the search_func_t signature has no in-band error channel (the reference's functions
 * print to stderr and return a partial count, e.g. krep.c:1359-1362), and a backend that answers 0
 * when it could not look would turn "failed" into "no match".  So (SURVEY §8b "Errors"):
 *   - without a usable gfx950 device krep_gpu_available() is 0, krep_gpu_can_accelerate() is 0 and
 *     krep_gpu_select_search_algorithm() returns NULL: the caller keeps the CPU function pointer the
 *     reference's own select_search_algorithm() gives it (krep.c:1944-1948);
 *   - an operator that fails at run time (allocation, copy, launch, device lost) appends NOTHING to
 *     `result`, prints "krep-gpu: ..." to stderr, sets krep_gpu_last_error() and
 *     krep_gpu_last_status() != 0, and — when the host registered its CPU selector with
 *     krep_gpu_set_cpu_fallback() — re-runs the search through the host's own CPU function and returns
 *     THAT result (status KREP_GPU_FELL_BACK).  Without a registered selector it returns 0 with status
 *     KREP_GPU_FAILED, which the caller must test (the error_flag path of krep.c:2940-2947).
 * search_buffer() returns 0 match / 1 no match / 2 error exactly like search_file()/search_string()
 * (krep.h:159,168).  The library itself contains no CPU implementation of any search: a fallback is
 * always the CALLER's function.  (krep_gpu_regex_compile() asks libc's regcomp / regexec which bytes each one-byte atom of a
 * pattern matches — 256 one-byte probes per atom, while the plan is made; that is a table, no search of a text.)
 */
#ifndef KREP_GPU_H
#define KREP_GPU_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef KREP_H /* ---- ABI twins of the reference types (krep.h:49-101) ---- */
typedef struct
{
    size_t start_offset; /* first byte of the match, relative to text_start           */
    size_t end_offset;   /* one past the last byte (exclusive)                         */
} match_position_t;      /* 16 bytes — also the record format the kernels write in HBM */

typedef struct match_result_t
{
    match_position_t *positions; /* malloc-family block: match_result_free() (krep.c:244) frees it */
    uint64_t count;
    uint64_t capacity;
} match_result_t;

struct ac_trie;
typedef struct ac_trie ac_trie_t;

typedef struct search_params
{
    const char *pattern; /* valid when num_patterns == 1 (krep.c:3736-3740) */
    size_t pattern_len;
    const char **patterns;
    size_t *pattern_lens;
    size_t num_patterns;
    bool case_sensitive;
    bool use_regex;
    bool count_lines_mode;
    bool count_matches_mode;
    bool track_positions;
    bool whole_word;
    const void *compiled_regex; /* const regex_t* in krep.h; never dereferenced here */
    ac_trie_t *ac_trie;         /* opaque; only tested against NULL (aho_corasick.c:306) */
    size_t max_count;
} search_params_t;

typedef uint64_t (*search_func_t)(const search_params_t *params, const char *text_start,
                                  size_t text_len, match_result_t *result);
#endif /* KREP_H */

/* ------------------------------------------------------------------------------------------------
 * Which reference build are we a drop-in for?  The reference picks its algorithm — and with it the
 * match-set family (all occurrences vs. greedy non-overlapping) — from compile-time SIMD macros
 * (krep.c:47-74, :1798-1869) and three file-static globals that no external backend can see
 * (krep.c:117-120).  They are made explicit here.  Defaults: AVX2 build, no overrides.
 * ---------------------------------------------------------------------------------------------- */
enum krep_ref_simd
{
    KREP_REF_SCALAR = 0, /* no -msse4.2: BMH / KMP / memchr only                   */
    KREP_REF_SSE42 = 1,  /* Makefile:40                                            */
    KREP_REF_AVX2 = 2,   /* Makefile:37                                            */
    KREP_REF_AVX512 = 3, /* Makefile:35                                            */
    KREP_REF_NEON = 4    /* Makefile:44-48 (arm64)                                 */
};
enum krep_ref_algo_override
{
    KREP_ALGO_AUTO = 0,
    KREP_ALGO_BM = 1, /* --algo=bm  (krep.c:1788) */
    KREP_ALGO_KMP = 2 /* --algo=kmp (krep.c:1790) */
};
/* The reference algorithm whose exact output (count, positions, order, max_count quirks) a scan
 * reproduces.  krep_gpu_mirror_select() is the twin of select_search_algorithm() incl. the
 * delegation chain AVX-512 -> AVX2 -> SSE4.2 -> BMH (krep.c:4708-4712, :4883-4896, :5114-5126). */
enum krep_ref_algo
{
    KREP_RA_NONE = 0,
    KREP_RA_BMH = 1,          /* boyer_moore_search   krep.c:1260 */
    KREP_RA_KMP = 2,          /* kmp_search           krep.c:1628 */
    KREP_RA_MEMCHR = 3,       /* memchr_search        krep.c:3891 */
    KREP_RA_MEMCHR_SHORT = 4, /* memchr_short_search  krep.c:4371 */
    KREP_RA_SSE42 = 5,        /* simd_sse42_search    krep.c:4702 */
    KREP_RA_AVX2 = 6,         /* simd_avx2_search     krep.c:4877 (17..32 B body) */
    KREP_RA_AVX512 = 7,       /* simd_avx512_search   krep.c:5108 (33..64 B body) */
    KREP_RA_NEON = 8,         /* neon_search          krep.c:4506 */
    KREP_RA_AHO_CORASICK = 9, /* aho_corasick_search  aho_corasick.c:299 */
    KREP_RA_REGEX = 10        /* regex_search         krep.c:1389 — the fixed-length class sequences of
                                 krep_gpu_regex_compile() below, their alternations (krep_gpu_regex_compile_alt())
                                 and what krep_gpu_regex_compile_ext() expands into one; everything else stays on the CPU */
};

/* All of it in one explicit object.  Plans and search_buffer_ex() carry their configuration; the setters below write the
 * PROCESS-WIDE defaults (like the reference's globals, set once by main() before the pool threads start; relaxed atomics),
 * krep_gpu_set_thread_config() overrides them for the calling thread (NULL: back to the defaults).  No scan path writes
 * any of this, so concurrent calls with different configurations do not interfere. */
typedef struct krep_gpu_config
{
    int reference_simd;        /* enum krep_ref_simd: which reference BUILD is reproduced (krep.c:47-74)              */
    int only_matching;         /* static only_matching (-o), krep.c:117                                                 */
    int force_no_simd;         /* static force_no_simd, krep.c:118                                                      */
    int algo_override;         /* enum krep_ref_algo_override (--algo), krep.c:120                                      */
    int result_order;          /* 1: multi-pattern records come back in (start, end) order (see below)                  */
    int device;                /* HIP device the host-buffer operators use (default: $KREP_GPU_DEVICE, else 0)          */
    size_t stream_chunk_bytes; /* piece size of the streamed host path (0 = default 128 MiB); texts > 2 pieces stream   */
    int num_gpus;              /* devices the search_func_t operators shard a text over (default: $KREP_GPU_NUM, else 1;
                                  0 or less = all visible devices); shards meet in one RCCL all-reduce of their counters  */
    size_t min_text_bytes;     /* krep_gpu_worthwhile(): texts shorter than this stay on the CPU function (default:
                                  $KREP_GPU_MIN_BYTES, else 1 MiB — one operator call costs 50-80 us)       */
} krep_gpu_config_t;
void krep_gpu_config_default(krep_gpu_config_t *out);           /* the current process-wide defaults */
void krep_gpu_set_thread_config(const krep_gpu_config_t *cfg);  /* calling thread only; NULL clears   */
void krep_gpu_set_device(int device);                           /* process-wide default device         */
void krep_gpu_set_stream_chunk(size_t bytes);                   /* process-wide default piece size     */
void krep_gpu_set_num_gpus(int n);                              /* process-wide default shard count    */
void krep_gpu_set_min_text_bytes(size_t bytes);                 /* process-wide default size threshold */
/* frees every per-device context of the host path (device buffers, pinned staging ring, cached plans) */
void krep_gpu_release_device_resources(void);

void krep_gpu_set_reference_simd(int krep_ref_simd_level);   /* compile-time SIMD macros, krep.c:47-74 */
void krep_gpu_set_only_matching(int on);                     /* static only_matching,   krep.c:117   */
void krep_gpu_set_force_no_simd(int on);                     /* static force_no_simd,   krep.c:118   */
void krep_gpu_set_algo_override(int krep_ref_algo_override); /* static algo_override,   krep.c:120   */
int krep_gpu_get_reference_simd(void);
/* Twin of select_search_algorithm() (krep.c:1771): the algorithm the reference build would END UP
 * executing for `params` on a text of `text_len` bytes (text_len matters: the SIMD functions fall back
 * to BMH when text_len < pattern_len, and so on). */
int krep_gpu_mirror_select(const search_params_t *params, size_t text_len);
const char *krep_gpu_algorithm_name(int krep_ref_algo); /* twin of get_algorithm_name(), krep.c:1964 */

/* ------------------------------------------------------------------------------------------------
 * Availability, failure status and the CPU fallback (SURVEY §8b "Errors", §5 "Failure detection").
 * ---------------------------------------------------------------------------------------------- */
/* 1 when the configured device exists, is a gfx950 and a probe kernel of this library's code object ran on it
 * (checked once per device and process); 0 otherwise, with the reason in krep_gpu_unavailable_reason().
 * $KREP_GPU_DISABLE=1 forces 0. */
int krep_gpu_available(void);
const char *krep_gpu_unavailable_reason(void); /* "" when available */
/* The host's own selector of CPU functions — for the reference CLI a wrapper of select_search_algorithm() (krep.c:1771)
 * that skips the GPU branch.  When registered, an operator that fails at run time calls
 * select_cpu(params)(params, text, len, result) itself and returns that function's result (sorted into (start, end)
 * order when result_order is set, so the promise of krep_gpu_set_result_order() holds either way). NULL unregisters. */
typedef search_func_t (*krep_gpu_cpu_select_t)(const search_params_t *params);
void krep_gpu_set_cpu_fallback(krep_gpu_cpu_select_t select_cpu);
/* Outcome of the calling thread's LAST operator / search_buffer call. */
enum krep_gpu_status
{
    KREP_GPU_OK = 0,        /* the scan ran on the GPU; the return value and `result` are the backend's             */
    KREP_GPU_FELL_BACK = 1, /* the GPU path failed; the registered CPU function produced the return value / result */
    KREP_GPU_FAILED = 2     /* the GPU path failed and no CPU function was available: the returned 0 means
                               "could not look", NOT "no match" — nothing was appended to `result`                 */
};
int krep_gpu_last_status(void);
/* Should a caller hand THIS text to the backend?  search_file() asks this once per file (krep.c:2404-2420 already special-cases
 * small files; krep.c:2729-2770 scales its thread count with the size).  1 iff
 *   text_len >= min_text_bytes  &&  krep_gpu_can_accelerate(params)  &&  the cost model expects the GPU to be faster  &&
 *   krep_gpu_available()   (asked last: a text that stays on the CPU never starts the HIP runtime).
 * The cost model (krep_amd/csrc/kg_cost.hip):
 *   t_gpu = (device not yet initialised in this process ? gpu_init_ms : 0) + gpu_launch_us + text_len / host-path rate
 *   t_cpu = text_len / min(cpu_threads x per-thread rate of the function select_search_algorithm() would run, its cap)
 * cpu_threads <= 0: what search_file() itself would use, min(cores, text_len / 4 MiB), at least 1 (krep.c:2748-2759).
 * The host-path rate is calibrated per process by the library itself (large operator calls after the first one, which also pays
 * for tables, arena and staging ring); the device-start term is dropped once the availability probe has run in this process (its
 * measured time is not used as a value).  Everything is overridable: krep_gpu_set_cost_rates(), $KREP_GPU_COST
 * ("host=50,launch=100,init=450,memchr=12:180,simd=6:150,scalar=1.5:100,ac=0.4:100": GB/s per thread : cap).
 * rates.enabled = 0 or $KREP_GPU_COST_MODEL=0: size and input class alone decide (the round-3 rule). */
typedef struct krep_gpu_cost_rates
{
    int enabled;
    double gpu_host_path_gbps, gpu_launch_us, gpu_init_ms;
    double cpu_memchr_gbps, cpu_memchr_cap_gbps;  /* memchr_search                                                  */
    double cpu_simd_gbps, cpu_simd_cap_gbps;      /* simd_sse42 / avx2 / avx512 / neon_search, memchr_short_search  */
    double cpu_scalar_gbps, cpu_scalar_cap_gbps;  /* boyer_moore_search, kmp_search                                 */
    double cpu_ac_gbps, cpu_ac_cap_gbps;          /* aho_corasick_search while its automaton fits the caches ...    */
    double cpu_ac_cache_bytes, cpu_ac_exponent;   /* ... and x (cache / automaton bytes)^exponent beyond (2 KiB per state) */
} krep_gpu_cost_rates_t;
typedef struct krep_gpu_cost
{
    double gpu_seconds, cpu_seconds;  /* the two estimates                                                  */
    double gpu_host_path_gbps;        /* the host-path rate used (calibrated when this process has measured one) */
    int cpu_threads, cpu_algo;        /* threads assumed; enum krep_ref_algo of the CPU function             */
    int device_ready;                 /* 1: this process has already started its device (no init in t_gpu)  */
} krep_gpu_cost_t;
int krep_gpu_worthwhile(const search_params_t *params, size_t text_len);
int krep_gpu_worthwhile_ex(const search_params_t *params, size_t text_len, int cpu_threads);
int krep_gpu_cost_estimate(const search_params_t *params, size_t text_len, int cpu_threads, krep_gpu_cost_t *out); /* 0 ok */
void krep_gpu_get_cost_rates(krep_gpu_cost_rates_t *out);
void krep_gpu_set_cost_rates(const krep_gpu_cost_rates_t *rates); /* NULL: back to the defaults + $KREP_GPU_COST */

/* ------------------------------------------------------------------------------------------------
 * Operator-level entry points (search_func_t-compatible).  `text_start` is a HOST pointer, exactly
 * as in the reference; the bytes are staged to HBM through pinned buffers, scanned by the HIP
 * kernels, and the results appended to `result` with the match_result_add() contract
 * (krep.c:175-241: malloc/realloc'd block, offsets relative to text_start, end exclusive).
 * Return value = match count, or distinct-line count when params->count_lines_mode.
 * ---------------------------------------------------------------------------------------------- */
uint64_t krep_gpu_literal_search(const search_params_t *params, const char *text_start,
                                 size_t text_len, match_result_t *result);
uint64_t krep_gpu_aho_corasick_search(const search_params_t *params, const char *text_start,
                                      size_t text_len, match_result_t *result);
/* regex_search (krep.c:1389-1579) for the patterns krep_gpu_regex_compile_anchored(), krep_gpu_regex_compile_alt() or
 * krep_gpu_regex_compile_ext() accepts; params->compiled_regex is never read here
 * and goes to the registered CPU function untouched when the attempt fails. */
uint64_t krep_gpu_regex_search(const search_params_t *params, const char *text_start,
                               size_t text_len, match_result_t *result);
/* Drop-in for select_search_algorithm(): returns one of the three functions above, or NULL when the backend does not
 * take the search — no usable device (krep_gpu_available() == 0), a regex all -E compilers refuse, and the input classes
 * krep_gpu_can_accelerate() names — so that the caller keeps the CPU function pointer the reference's own
 * select_search_algorithm() gives it.  (-c through simd_sse42_search / kmp_search with a newline inside the pattern, refused
 * until round 3, is reproduced: one device thread walks the ordered occurrence list the way the reference's loop moves.) */
search_func_t krep_gpu_select_search_algorithm(const search_params_t *params);
/* 1 when the backend takes the search for `params` under the current configuration, 0 when not:
 *   - no usable gfx950 device (krep_gpu_available() == 0);
 *   - no pattern at all (num_patterns == 0 and pattern == NULL);
 *   - use_regex with a search krep_gpu_regex_compile_anchored(), krep_gpu_regex_compile_alt() and krep_gpu_regex_compile_ext()
 *     all refuse (anything that is neither a fixed number of byte classes in a row with an optional ^ in front and $ behind nor
 *     an alternation of such sequences nor an expression of ?, {n,m} and groups that expands into one; -w).  The reason reported
 *     is the alternation compiler's when the search says an alternation (several patterns, or a '|' or '(' outside brackets and
 *     not behind a backslash), else the anchored compiler's; krep_gpu_regex_compile_ext()'s when only its own limits refuse.
 *     With krep_gpu_set_regex_loops(1) krep_gpu_regex_compile_loops() is asked fourth, with krep_gpu_set_regex_groups(1)
 *     krep_gpu_regex_compile_groups() fifth (both off by default): a search one of them takes is taken, and their own reason
 *     replaces the earlier one only where their contracts below say so;
 * (count_lines_mode together with only_matching through memchr_short_search — a combination krep's main() never produces,
 * krep.c:3811-3814 — was refused until round 5 and is reproduced now: one window, krep_gpu_split_mode() = WHOLE.)
 * An operator called with such params anyway treats it like a run-time failure (see the top of this header): the
 * registered CPU function answers, or status KREP_GPU_FAILED; nothing is silently approximated. */
int krep_gpu_can_accelerate(const search_params_t *params);

/* ---- krep -E on the device: fixed-length class sequences ----
 * Most -E patterns are a fixed number of byte classes in a row (Sherl[oO]ck, [0-9]{3}-[0-9]{4}, 0x[0-9a-f]{8}); those are
 * scanned on the device, every other expression stays with krep's regex_search.  The compiler is a TOKENISER: it cuts
 * params->pattern (or patterns[0]) into atoms and interprets none of them.
 * Accepted atoms: an ordinary byte; '\' followed by a punctuation byte; '.'; a bracket expression, whose closing ']' is found
 *   by POSIX's rules (an optional '^', a ']' directly behind '[' or '[^' is literal, [:name:] [.x.] [=x=] are stepped over).
 *   Each atom may be followed by {n}, n >= 1, which repeats it.  The atoms in a row are the L byte classes C0..C(L-1), 1 <= L <= 16.
 * Refused (2, the reason in krep_gpu_last_error()): ( ) * + ? | outside brackets; ^ and $ outside brackets (as the first / last
 *   pattern byte they are line anchors: krep_gpu_regex_compile_anchored() below takes those); {n,} and {n,m}; '{' not behind an atom;
 *   '\' followed by a letter or digit (\b, \w, \1, ...); a pattern byte outside 0x01-0x7F; L outside 1..16; num_patterns > 1
 *   (the CLI turns several -e into an alternation); whole_word — the CLI compiles \bPATTERN\b (krep.c:2122-2135) and still calls
 *   is_whole_word_match(), a library caller compiles PATTERN alone, the operator sees only params->pattern and never the compiled
 *   expression, and the two forms disagree on real texts: there is no single behaviour to reproduce.  Also refused: every pattern
 *   while the process runs in a multibyte locale (MB_CUR_MAX > 1, a caller that called setlocale()): libc's regexec matches
 *   characters there — '.', a negated or named class and, under REG_ICASE, even a letter take a whole multibyte sequence as one
 *   atom — so nothing is a fixed number of byte classes.  krep itself never calls setlocale() and runs in the C locale.
 * Classes: every atom's substring is compiled ALONE with regcomp(REG_EXTENDED | REG_NEWLINE | (case_sensitive ? 0 : REG_ICASE)),
 *   the flags of krep.c:2148, and all 256 one-byte texts are put to regexec(REG_STARTEND): the class is what matched.  So the
 *   classes are those of the libc the caller's own regexec uses, wherever the library runs — in glibc's C locale '.' is 0x01-0x7F
 *   without '\n' (no NUL, no byte >= 0x80), [^a] holds NUL but no byte >= 0x80 and no '\n' and loses 'A' too under REG_ICASE,
 *   [[:space:]] holds '\n' — and no table written down here can be wrong about them.
 * What a scan reproduces (regex_search's REG_STARTEND loop, which resumes at the match's end, krep.c:1539-1568): an occurrence
 *   is a position p with text[p + j] in Cj for all j, p + L <= text_len.  Matches: the greedy leftmost non-overlapping
 *   occurrences, each (p, p + L).  -c: the distinct lines that hold the START of an occurrence (overlap does not matter: after a
 *   counted line the reference jumps to the next line start); a start ON a '\n' belongs to the line that newline ends.
 *   max_count: the return value is min(total, max_count), the records are the first max_count; max_count == 0 returns 0 when
 *   count_lines_mode or track_positions is set and otherwise 1 as soon as one occurrence exists (krep.c:1395, :1533).
 *   only_matching and reference_simd change nothing.
 * Split: a pattern that cannot overlap itself (self_overlap == 0: for no shift d in 1..L-1 do Cj and C(j+d) meet for every j),
 *   and every pattern under -c, is KREP_GPU_SPLIT_PIECES.  A self-overlapping pattern without -c goes through the greedy pass over
 *   the occurrence list: KREP_GPU_SPLIT_WHOLE, and a window that is not the whole text is refused (2). */
typedef struct krep_gpu_regex_info
{
    uint32_t L;               /* byte classes in a row, 1..16                                            */
    uint8_t classes[16][32];  /* class j as a 256-bit set: byte b is in it iff classes[j][b >> 3] >> (b & 7) & 1 */
    int self_overlap;         /* 1: two occurrences may overlap (the greedy pass decides which are matches)      */
    uint32_t anchor;          /* index of the class with the fewest bytes (the first such)                */
    uint8_t anchor_bytes[4];  /* its bytes, ascending, when there are at most 4 of them                   */
    uint32_t n_anchor;        /* how many of anchor_bytes are set; 0: the class holds more than 4 bytes (or none) */
} krep_gpu_regex_info_t;
/* Host only, needs no device.  Returns 0 and fills *out, or 2 with the reason in krep_gpu_last_error(). */
int krep_gpu_regex_compile(const search_params_t *params, krep_gpu_regex_info_t *out);

/* ---- line anchors around a class sequence: ^ERROR, ;$, ^#include$, [0-9]{3}$ ----
 * Grammar: an optional '^' as the first pattern byte, an optional '$' as the last one (when it is not the second byte of a \$
 *   escape), and between them exactly the grammar above.  \^, \$, [$^] and [^a] stay ordinary atoms.  krep_gpu_regex_compile()
 *   keeps refusing both anchors (its struct cannot say them); everything that takes a search — krep_gpu_can_accelerate(),
 *   krep_gpu_select_search_algorithm(), krep_gpu_split_mode(), the plans and the operators — goes through this call.
 * Refused (2, each with its own reason): '^' or '$' anywhere else outside a bracket (a^b, a$b, ^^a, a$$); {n} directly behind
 *   '^'; ^$, ^ and $ on their own (L = 0: an empty match); L + bol + eol > 16; and everything krep_gpu_regex_compile() refuses.
 * What a scan reproduces (regex_search under REG_EXTENDED | REG_NEWLINE, REG_NOTBOL unless the search resumes at the text start
 *   or behind a '\n', REG_STARTEND with rm_eo = the end of the text): an occurrence is a position p with
 *     text[p + j] in Cj for all j < L, and p + L <= text_len;
 *     when bol: p == 0 or text[p - 1] == '\n';
 *     when eol: text[p + L] == '\n', or p + L == text_len in a case-sensitive search.  (regex_search ORs REG_ICASE into regexec's
 *       eflags, krep.c:1420, where that bit is REG_NOTEOL: with case_sensitive == false the end of the text ends no line, and
 *       a$ does not match the text "a".  The scan reproduces that.)
 *   The anchors consume nothing: the records are (p, p + L), the matches the greedy leftmost non-overlapping occurrences with
 *   consume = L.  -c counts the distinct lines that hold p; a p ON a '\n' belongs to the line that newline ends.  max_count, its
 *   0 quirk, only_matching and the empty text are as above.
 * seq.self_overlap: a shift d in 1..L-1 counts only when Cj and C(j+d) meet for every j AND, with bol, C(d-1) holds '\n' (the byte
 *   in front of the second occurrence lies inside the first) AND, with eol, C(L-d) holds '\n'.  So ^ab, ab$ and ^[ab]{2} are
 *   KREP_GPU_SPLIT_PIECES, ^[a\n]{2} is KREP_GPU_SPLIT_WHOLE (without -c).
 * Windows: a scan needs text[p - 1] and text[p + L] of every start it owns.  Refused (2): bol with own_lo == 0 in a buffer that
 *   does not begin the text (global_base > 0); eol with an owned start at p + L == text_len in a buffer that does not end the text
 *   (global_base + text_len < global_len).  The pieces the library cuts itself carry 17 bytes on both sides and never ask that. */
typedef struct krep_gpu_regex_anchored
{
    krep_gpu_regex_info_t seq; /* the L real classes; anchor / anchor_bytes / n_anchor as above, over the real classes */
    int bol;                   /* the pattern starts with an unescaped ^ */
    int eol;                   /* the pattern ends with an unescaped $   */
} krep_gpu_regex_anchored_t;
/* Host only, needs no device.  Returns 0 and fills *out, or 2 with the reason in krep_gpu_last_error(). */
int krep_gpu_regex_compile_anchored(const search_params_t *params, krep_gpu_regex_anchored_t *out);

/* ---- alternations of class sequences: ERROR|WARN|FATAL, cat|d[oi]g|b.rd, and every -E run with several -e ----
 * Grammar: every pattern of params (patterns[0..num_patterns), or pattern alone) is B ( '|' B )*, each B either a class sequence
 *   of the unanchored grammar above or one such sequence inside exactly one pair of parentheses, (Sherl[oO]ck).  The branches of
 *   all patterns together are the alternation: that is what the CLI's (p1)|(p2) means.  '|', '(' and ')' inside a bracket
 *   expression or behind a backslash stay ordinary.  Branches whose class tables are identical are merged.
 * Refused (2, each with its own reason): an empty branch (a|, |a, (), a||b: it matches the empty string); nested or unbalanced
 *   parentheses; a group that is not a whole branch (x(a|b)y, (ab)c, (ab){2}, (a|b)); ^ or $ in any branch; more than 8 branches
 *   after merging; a branch of more than 16 classes; total_L > 32; and everything krep_gpu_regex_compile() refuses in a branch.
 *   krep_gpu_regex_compile() and krep_gpu_regex_compile_anchored() keep refusing '|', '(', ')' and several patterns: everything that
 *   takes a search asks the anchored compiler first and this one only when that one refuses, so a pattern accepted there runs
 *   the kernel it always ran.
 * What a scan reproduces (regex_search, checked against the compiled reference with a brute-force model): branch i with classes
 *   C[i][0..L_i) occurs at p when text[p + j] is in C[i][j] for all j and p + L_i <= text_len.  The occurrence at p is
 *   (p, p + len(p)), len(p) the LONGEST L_i among the branches that occur at p (POSIX leftmost-longest: ab|abc on xabcabx gives
 *   (1,4),(4,6)).  Matches: the greedy leftmost non-overlapping selection over the positions that hold an occurrence, consuming
 *   len(p) (a|aa on aaaaa gives (0,2),(2,4),(4,5)); records ascend in start.  -c: the distinct lines that hold the start of any
 *   branch's occurrence (no greedy selection: after a counted line the reference jumps to the next line start); a start ON a
 *   '\n' belongs to the line that newline ends.  max_count, its 0 quirk, only_matching and reference_simd as above.
 * cross_overlap: 1 iff there are branches i, j and a shift d, 0 <= d < L_i (d >= 1 when i == j), such that C[i][d + t] meets
 *   C[j][t] for every t with d + t < L_i and t < L_j: two occurrences can share a byte (d == 0 with i != j is the same start).
 * Split: -c is always KREP_GPU_SPLIT_PIECES; without -c PIECES when cross_overlap == 0, else KREP_GPU_SPLIT_WHOLE (the greedy
 *   pass runs over the whole occurrence list, and a window that is not the whole text is refused (2)).  Halo and shards use
 *   Lmax <= 16 where a single sequence uses L. */
typedef struct krep_gpu_regex_alt
{
    uint32_t n_branches;             /* 1..8, after identical branches have been merged              */
    uint32_t Lmin, Lmax, total_L;    /* over the branches; every L in 1..16, total_L <= 32            */
    int cross_overlap;               /* 1: two occurrences (of one branch or of two) can share a byte */
    uint32_t reserved;
    krep_gpu_regex_info_t branch[8]; /* each exactly what krep_gpu_regex_compile() makes of the branch alone */
} krep_gpu_regex_alt_t;
/* Host only, needs no device.  Returns 0 and fills *out, or 2 with the reason in krep_gpu_last_error(). */
int krep_gpu_regex_compile_alt(const search_params_t *params, krep_gpu_regex_alt_t *out);

/* ---- ?, {n,m}, inner groups and anchored alternations: colou?r, [0-9]{1,3}%, (GET|POST) /api, ^(ERROR|WARN), \.(jpg|png)$ ----
 * Each of these is a finite set of fixed-length class sequences between one pair of line anchors.  This compiler EXPANDS the
 * expression into that set; the scan is the alternation's, with ^ and $ as one more place in front of and behind every branch.
 * Grammar: every pattern of params is B ( '|' B )*, the top-level branches of all patterns together being the alternation.
 *   B     = ['^'] item+ ['$']
 *   item  = atom quant? | group quant?
 *   atom  = what krep_gpu_regex_compile() takes as one: an ordinary byte, '\' + punctuation, '.', a bracket expression
 *   group = '(' seq ( '|' seq )* ')',  seq = ( atom quant? )+      (no group inside a group, no ^ or $ inside a group)
 *   quant = '?' | '{n}' | '{n,m}'  with 0 <= n <= m and m >= 1
 *   A branch expands to the product of its items' alternatives (colou?r: color, colour; (ab){2}: abab; x(a|bc)y: xay, xbcy);
 *   sequences whose class tables are identical merge.  ^ and $ are anchors only as the first and the last byte of a top-level
 *   branch, and every branch of every pattern must carry the same pair: ^(a|b), ^a|^b and -e '^GET' -e '^POST' are taken,
 *   ^a|b and -e a -e '^b' are not.
 * Refused (2, each with its own reason): * + and {n,}; a quantifier behind a quantifier; an expansion that holds an empty
 *   sequence (a?, (a|b)?, a{0}, ^$); an empty alternative in a group or an empty branch; nested or unbalanced parentheses; ^ or $
 *   inside a group or in the middle of a branch; mixed anchors; more than 8 distinct sequences; a sequence with L + bol + eol > 16;
 *   the sum of L + bol + eol over the sequences > 32; -w; a multibyte locale; a pattern byte outside 0x01-0x7F; an atom the
 *   tokeniser refuses.
 * Every search asks krep_gpu_regex_compile_anchored() first, then krep_gpu_regex_compile_alt(), then this call (and, behind their
 *   switches, krep_gpu_regex_compile_loops() and krep_gpu_regex_compile_groups() below): a search one of
 *   those takes runs the kernel it always ran.  The reason reported for a search all three refuse is the one reported before
 *   this compiler existed, unless the search fails only at this compiler's own limits (the number of sequences or places after
 *   expansion, an empty sequence in the expansion): then it is this compiler's.
 * What a scan reproduces (regex_search; checked against glibc with a brute-force model): branch i with classes C[i][0..L_i)
 *   occurs at p when text[p + j] is in C[i][j] for all j < L_i, p + L_i <= text_len;
 *     when bol: p == 0 or text[p - 1] == '\n';
 *     when eol: text[p + L_i] == '\n', or p + L_i == text_len in a case-sensitive search (the REG_NOTEOL quirk described above).
 *   The occurrence at p is (p, p + the longest occurring L_i); the matches are the greedy leftmost non-overlapping selection that
 *   consumes that length; the anchors consume nothing.  -c counts the distinct lines that hold an occurrence's start.  max_count
 *   and its 0 quirk as above.
 * alt: the expanded branches over the REAL classes, each what krep_gpu_regex_compile() makes of that sequence alone; Lmin, Lmax
 *   and total_L over the real lengths.  alt.cross_overlap is computed over the expanded set: branches i, j and a shift d as above,
 *   where for d >= 1 an anchor rules the pair out when the newline it needs falls on a class that holds none (under ^ the byte in
 *   front of the second occurrence, class C[i][d - 1]; under $ the byte behind the occurrence that ends first).  The same start
 *   on two branches (d == 0) always counts.  Split and windows: as for an alternation and for an anchored sequence — -c is
 *   KREP_GPU_SPLIT_PIECES, without -c PIECES when cross_overlap == 0 and else WHOLE; bol with own_lo == 0 in a buffer that does not
 *   begin the text and eol with an owned occurrence that ends on the last byte of a buffer that does not end the text are
 *   refused (2). */
typedef struct krep_gpu_regex_ext
{
    krep_gpu_regex_alt_t alt; /* the expanded set over the real classes                  */
    int bol;                  /* every top-level branch starts with an unescaped ^       */
    int eol;                  /* every top-level branch ends with an unescaped $         */
} krep_gpu_regex_ext_t;
/* Host only, needs no device.  Returns 0 and fills *out, or 2 with the reason in krep_gpu_last_error(). */
int krep_gpu_regex_compile_ext(const search_params_t *params, krep_gpu_regex_ext_t *out);

/* ---- *, + and {n,} behind an atom: ERROR.*timeout, [0-9]+\.[0-9]+, [a-z]+@[a-z]+\.com, colou*r, ^#+ ----
 * Grammar: krep_gpu_regex_compile_ext()'s, with three more quantifiers behind an ATOM (at top level or inside a group's alternative):
 *   quant = '?' | '{n}' | '{n,m}' | '*' | '+' | '{n,}'
 *   A PLACE of a sequence is a byte class plus a flag "repeats": C+ is the place C that repeats, C{n,} is C n - 1 times and then C+, C*
 *   and C{0,} are {nothing, C+}.  Everything else expands as in krep_gpu_regex_compile_ext(); two sequences are the same when their
 *   classes and their flags are.  The limits are that compiler's: at most 8 sequences, at most 16 places each (^ and $ take one each),
 *   at most 32 in all.
 * Refused (2, each with its own reason): an unbounded quantifier behind a group ((ab)+, (a|b)*); any class of the program that holds
 *   '\n' ([^a]+ does not, [[:space:]]+ does); an expansion that holds an empty sequence (a*, a*b*); an expression without any *, + or
 *   {n,} (the older compilers keep what is theirs); and everything krep_gpu_regex_compile_ext() refuses for other reasons.
 * The filter.  For a branch with places p0..p(L-1) a FACTOR is a run pa..pb in which no place strictly between a and b repeats (a
 *   repeating place may stand at either end: it gives the one byte of its run that touches its neighbour).  Every text the branch
 *   matches holds every factor as consecutive bytes.  Per branch the factor with the smallest product of |class| / 256 is taken, on
 *   a tie the longer one, then the leftmost; identical factors merge.  `filter` is that unanchored alternation of at most 8 sequences of
 *   at most 16 classes, which the fixed-length kernels scan: a+b gives ab, [0-9]+ gives [0-9], ERROR.*timeout expands into ERRORtimeout
 *   and ERROR.+timeout and gives ERRORtimeout and .timeout.
 * What a scan reproduces (regex_search under REG_NEWLINE, checked against the compiled reference with a brute-force model), per line.
 *   The lines are [0, first '\n'), every stretch between two newlines and what stands behind the last newline, if that is not empty.
 *   In a line [ls, le), with resume = ls:
 *     a start s >= resume is tried in ascending order; with bol only s = ls;
 *     a branch matches (s, e) when text[s, e) can be cut into non-empty runs, one per place and in order, each of bytes of its place's
 *       class, of length 1 unless the place repeats, and e <= le;
 *     with eol e must be le; when le is the end of the text and not a newline that holds only in a case-sensitive search (the
 *       REG_NOTEOL quirk described above);
 *     the match at s is (s, the largest such e over all branches); the first s that has one is emitted and resume moves to its e.
 *   Records ascend in start.  -c counts the lines that hold a match.  max_count, its 0 corner and the empty text as above;
 *   only_matching and reference_simd change nothing.
 * Split: KREP_GPU_SPLIT_WHOLE.  A window that is not the whole text is refused (2).  That is the default; with
 *   krep_gpu_set_regex_loops_windows(1) it is KREP_GPU_SPLIT_PIECES:
 *   Ownership.  A window reports the matches of the whole text whose START lies in its owned range, global_base + [own_lo, own_hi);
 *     the lists of adjacent windows concatenate to the whole-text list.  A line's walk still starts at the line's first byte — the
 *     matches in front of own_lo decide where the first owned attempt stands — so the buffer must hold every line that meets the
 *     owned range, whole.  A finite max_count gives each window its own first max_count records.  -c counts the lines that hold an
 *     owned start; head_line_hit / tail_line_hit / has_newline mean what every other scan's mean (a counted line that began at or in
 *     front of own_lo, one that ends at or behind own_hi, a '\n' inside the owned range), and krep_gpu_combine_line_counts() folds the
 *     windows.  krep_gpu_scan_device_seq() passes its boundary record through: the family has no sequential dependency.
 *   Context.  No line of more than 4096 bytes is ever walked, so 4096 bytes of the text on each side of the owned range (fewer where
 *     the text begins or ends) hold every such line.  Two refusals (2, nothing written): a line that meets the owned range and is
 *     longer than 4096 bytes as far as the buffer shows it ("a line of more than 4096 bytes"), and a line that meets the owned range,
 *     is at most that long, and touches an end of the buffer that is not an end of the text ("the window does not hold the whole of a
 *     line that meets its owned range").  A cut line in the context that does not meet the owned range is not looked at.  The line
 *     the buffer's END cuts is held to this rule whether or not the buffer shows a filter occurrence in it: the occurrence of a match
 *     that starts in the owned range may lie behind that end.
 *   The road is chosen per buffer.  The filter scan, its 1/64 density rule and the line analysis run over the buffer, not over the
 *     owned range, so whether a long line that holds no filter occurrence is met at all depends on the road each buffer takes: a
 *     scan in pieces may refuse a text for a line of more than 4096 bytes where the one-window scan took the sparse road and never
 *     looked at that line.  The host operators answer identically either way: the registered CPU function takes over.
 *   The host executor stages each piece with 4097 bytes on both sides, shards such a search over num_gpus and streams it.
 * Long lines: a lane of the device walks one line, and its worst case is quadratic in the line's length (a.*b on a line of a's).  A
 *   candidate line of more than 4096 bytes is not walked: the scan returns 2 ("a line of more than 4096 bytes") with nothing
 *   written, and the operator takes the road of every run-time failure (the registered CPU function, or KREP_GPU_FAILED).
 *   krep_gpu_set_regex_long_lines(1) (process-wide, off unless $KREP_GPU_REGEX_LONG_LINES=1 is set when the library is loaded; it
 *   matters only to a search this compiler or the groups compiler took) lifts that rule for the scan of the WHOLE text in one
 *   window, batch packs included: a candidate line of more than 4096 bytes is walked by one lane in two linear passes, a backward
 *   pass that marks in one 32-bit word per line byte the places that still reach a match's end from there and the forward
 *   leftmost-longest walk pruned by those words — about three steps per byte whatever the expression, the same records and counts.
 *   The words live in device scratch the plan keeps, at most 256 MiB of them (64 Mi line bytes) plus one line; when a text's long
 *   candidate lines need more they are walked in rounds.  The rule that stays: one line of more than 1 MiB (min(1 MiB, budget / 4))
 *   returns 2 with the same sentence and that number in it.  Any other window keeps the 4096-byte rule and its two refusals whatever
 *   krep_gpu_set_regex_loops_windows() says — the 4096 bytes of context rest on it —, so the sharded and the streaming executor
 *   and the pieces drivers do too.  The switch changes nothing in krep_gpu_can_accelerate(), krep_gpu_split_mode() or the plan's
 *   longest match (4097 for such a search).  Off, every call answers and reports as if it did not exist.
 * The switch.  krep_gpu_regex_compile_loops() always works.  Whether a SEARCH asks it, last, after the three older compilers have
 *   refused, is decided by krep_gpu_set_regex_loops(): process-wide, off unless $KREP_GPU_REGEX_LOOPS=1 is set when the library is
 *   loaded.  Off, every call behaves and reports as if this compiler did not exist.  On, krep_gpu_can_accelerate(), the selector, the
 *   plans, krep_gpu_regex_search, search_buffer and the batch calls take such a search; a search all four refuse reports what it
 *   reported before, unless that was a "repeat without a bound" reason: then it is this compiler's. */
typedef struct krep_gpu_regex_loops
{
    krep_gpu_regex_alt_t alt;    /* the expanded sequences over their real classes; L, Lmin, Lmax, total_L count PLACES, not bytes;
                                    cross_overlap / self_overlap are those of the places read as single bytes: no scan uses them */
    int bol;                     /* every top-level branch starts with an unescaped ^ */
    int eol;                     /* every top-level branch ends with an unescaped $   */
    uint16_t repeat[8];          /* bit j of repeat[i]: place j of alt.branch[i] repeats (C+) */
    krep_gpu_regex_alt_t filter; /* the factors, each branch what krep_gpu_regex_compile() makes of that sequence alone */
} krep_gpu_regex_loops_t;
/* Host only, needs no device.  Returns 0 and fills *out, or 2 with the reason in krep_gpu_last_error(). */
int krep_gpu_regex_compile_loops(const search_params_t *params, krep_gpu_regex_loops_t *out);
void krep_gpu_set_regex_loops(int on); /* process-wide; default 0, or $KREP_GPU_REGEX_LOOPS at load */
int krep_gpu_get_regex_loops(void);
/* Windows of such a search ("Split" above): process-wide; default 0, or $KREP_GPU_REGEX_LOOPS_WINDOWS at load.  Off, or with
 * krep_gpu_set_regex_loops() off, every call answers as if this switch did not exist. */
void krep_gpu_set_regex_loops_windows(int on);
int krep_gpu_get_regex_loops_windows(void);
/* Lines of more than 4096 bytes of such a search ("Long lines" above): process-wide; default 0, or $KREP_GPU_REGEX_LONG_LINES at load */
void krep_gpu_set_regex_long_lines(int on);
int krep_gpu_get_regex_long_lines(void);

/* ---- repeated and nested groups: (ab)+, (foo|bar)+;, ([a-z]+\.)+com, ((GET|POST) |HEAD )/api, [0-9]{1,3}\.[0-9]{1,3}\.… ----
 * The four compilers above expand an expression into at most 8 flat sequences.  This one does not expand: it holds the expression
 *   as its POSITION (Glushkov) automaton, one bit per atom occurrence.
 * Grammar: krep_gpu_regex_compile_loops()'s with groups made recursive:
 *   item = atom quant? | '(' alt ')' quant?      alt = seq ('|' seq)*      seq = item+
 *   quant = '?' | '*' | '+' | '{n}' | '{n,}' | '{n,m}', behind atoms and behind groups; parentheses nest to depth 8.
 *   Atoms are the tokeniser's, their classes probed from libc.  ^ and $ are taken only as the first and the last byte of a top-level
 *   branch, the same pair on every top-level branch of every pattern; they take no position (the line walk owns them).
 * Positions.  A counted quantifier copies its operand: X{2,} is X X+, X{1,3} is X X? X?, X{0,} is X*.  The positions are the atom
 *   occurrences after that copying, numbered left to right, at most 32.  classes[i] is the class of position i; first / last are
 *   the positions a match can start / end on; follow[i] the positions that can stand directly behind position i.
 * Refused (2, each with its own reason): a class that holds '\n'; an expression that matches the empty string (a nullable
 *   sub-expression inside a whole that is not — x(ab)*y, (a*b)+ — is taken); an empty alternative or an empty group; a quantifier
 *   behind a quantifier or behind nothing; {0} and {0,0}; ^ or $ anywhere else; top-level branches with different anchors; more than 32
 *   positions; nesting deeper than 8; a follow relation of more than 12 jump pairs (below); an expression without a filter (below);
 *   -w; a multibyte locale; a pattern byte outside 0x01-0x7F; an atom the tokeniser refuses; and an expression one of the four older
 *   compilers takes: they keep what is theirs.
 * Jump pairs.  The line walk steps follow(S) = ((S & CHAIN) << 1) | (S & SELF) | the targets of every pair whose sources meet S:
 *   CHAIN the positions i with i + 1 in follow[i] (never position 31), SELF those with i in follow[i]; what is left of a follow set
 *   is a jump (source mask, target mask), and positions with the same remainder share a pair.  At most 12 pairs.
 * The filter: at most 8 class sequences of at most 16 classes, 32 classes in all, with ONE binding property: every match of the
 *   expression holds an occurrence of one of them as consecutive bytes.  It is derived from a set of positions that every match
 *   passes (an atom: itself; a concatenation: the best of its parts that are not nullable; an alternation: the union over its
 *   alternatives; X+ and X{n>=1,..}: that of X; a nullable part: none).  Each position's factor is its class lengthened along
 *   forced edges: forward while no position reached so far is in `last` and all positions that can follow have one and the same
 *   class, backward likewise with `first` and the predecessors.  Best is the smallest sum over the distinct factors of the product of
 *   |class| / 256; on a tie the set whose shortest factor is longer, then the leftmost.  The IP expression gives [0-9]\.[0-9].
 * What a scan reproduces: regex_search under REG_NEWLINE, per line, as krep_gpu_regex_compile_loops() states it ("What a scan
 *   reproduces" above), with "a branch matches (s, e)" read as: text[s, e) is accepted by the automaton — text[s] is in the class of a
 *   position of `first`, every next byte in the class of a position that follows the one before, the last one in `last`.  The match at
 *   s is (s, the largest such e): leftmost start, longest end over ALL paths, which is what glibc's regexec reports for these
 *   expressions (checked against the compiled reference with a brute-force model).
 * Windows, context, long lines and split are the loops compiler's, word for word: "Split", "Ownership", "Context", "Long lines" above,
 *   under the same switch krep_gpu_set_regex_loops_windows().
 * The switch.  krep_gpu_regex_compile_groups() always works.  A SEARCH asks it fifth, after the loops compiler, only when
 *   krep_gpu_set_regex_groups(1) is on: process-wide, off unless $KREP_GPU_REGEX_GROUPS=1 is set when the library is loaded, and
 *   independent of krep_gpu_set_regex_loops().  Off, every call behaves and reports as if this compiler did not exist.  On, a search
 *   all five refuse reports what it reported before, unless that was a reason about a group, about nesting or about what an
 *   expansion multiplies out to (a group that is not a whole branch, a group that holds an alternation, nested parentheses, a
 *   quantifier behind a group, more than 8 sequences, 16 places or 32 places after expansion): then it is this compiler's. */
typedef struct krep_gpu_regex_groups
{
    uint32_t n_pos;              /* positions, 1..32 */
    uint8_t classes[32][32];     /* classes[i]: the 256-bit class of position i */
    uint32_t first, last;        /* bit i: a match can start / end on position i */
    uint32_t follow[32];         /* follow[i] bit j: position j can stand directly behind position i */
    int bol;                     /* every top-level branch starts with an unescaped ^ */
    int eol;                     /* every top-level branch ends with an unescaped $   */
    krep_gpu_regex_alt_t filter; /* the factors, each branch what krep_gpu_regex_compile() makes of that sequence alone */
} krep_gpu_regex_groups_t;
/* Host only, needs no device.  Returns 0 and fills *out, or 2 with the reason in krep_gpu_last_error(). */
int krep_gpu_regex_compile_groups(const search_params_t *params, krep_gpu_regex_groups_t *out);
void krep_gpu_set_regex_groups(int on); /* process-wide; default 0, or $KREP_GPU_REGEX_GROUPS at load */
int krep_gpu_get_regex_groups(void);

/* The in-memory twin of search_file()/search_string() that BASELINE.json calls search_buffer():
 * validation as krep.c:2013-2049 (no patterns -> 2; empty pattern among several -> 2; pattern
 * longer than 1024 -> 2), algorithm selection as krep.c:2166, single-chunk semantics, clamp to
 * max_count as krep.c:2176-2184.  Nothing is printed.  num_gpus > 1 shards the buffer by contiguous
 * chunk across that many devices of this process with start-offset ownership.
 * Returns 0 = match found, 1 = none, 2 = error. */
int search_buffer(const search_params_t *params, const char *buf, size_t len, int only_matching,
                  int num_gpus, match_result_t *out /* nullable */, uint64_t *count_out /* nullable */);
/* The same with the whole configuration explicit (cfg == NULL: the calling thread's current configuration).
 * Re-entrant: any number of threads may call it concurrently with different configurations. */
int search_buffer_ex(const search_params_t *params, const char *buf, size_t len, const krep_gpu_config_t *cfg,
                     int num_gpus, match_result_t *out /* nullable */, uint64_t *count_out /* nullable */);

/* match_result_t helpers with the reference's allocation contract (krep.c:139-251), exported so a
 * caller without krep.c can own the results. */
match_result_t *krep_gpu_match_result_init(uint64_t initial_capacity);
void krep_gpu_match_result_free(match_result_t *r);

/* ------------------------------------------------------------------------------------------------
 * Device-resident path (the one the roofline number is measured on): the haystack already lives
 * in HBM.  A plan holds the compiled pattern set (pattern words / Aho-Corasick filter + trie
 * tables) on one device; a scan runs it over a device buffer.
 * ---------------------------------------------------------------------------------------------- */
typedef struct krep_gpu_plan krep_gpu_plan_t;

/* per-scan output; counters are exact even when the position buffer is too small */
typedef struct krep_gpu_scan_out
{
    uint64_t count;          /* what the reference function would RETURN for this shard           */
    uint64_t stored;         /* number of match_position_t records written to d_positions         */
    uint64_t total_matches;  /* uncapped number of emitted matches (before max_count)             */
    uint64_t line_count;     /* distinct lines holding a match start (count_lines_mode), shard-local */
    uint8_t head_line_hit;   /* a match starts before the first '\n' of the owned window           */
    uint8_t tail_line_hit;   /* a match starts after the last '\n' of the owned window             */
    uint8_t has_newline;     /* the owned window contains at least one '\n'                        */
    uint8_t overflow;        /* 1: more matches than position capacity (re-run with more)          */
    float kernel_ms;         /* hipEvent time of the scan kernels on `stream` (0 if not timed)     */
} krep_gpu_scan_out_t;

/* A plan is used by ONE thread at a time: it owns scratch buffers, events and what its scans have learnt about the text's density
 * (staging-slot size, ring shape of the one-pass kernels, which -c road pays off) — re-evaluated by every scan, not synchronised.
 * Concurrent scans take one plan each (the host operators keep a small plan cache per device behind the device's mutex). */
krep_gpu_plan_t *krep_gpu_plan_create(const search_params_t *params, int only_matching, int device);
krep_gpu_plan_t *krep_gpu_plan_create_ex(const search_params_t *params, const krep_gpu_config_t *cfg /* NULL = current */);
void krep_gpu_plan_destroy(krep_gpu_plan_t *plan);
int krep_gpu_plan_ref_algo(const krep_gpu_plan_t *plan); /* enum krep_ref_algo this plan reproduces */

/* Scan d_text[0 .. text_len) and report the matches whose START lies in [own_lo, own_hi)
 * (start-offset ownership; bytes outside the window are context: the tail halo completes matches
 * that begin inside, the byte before own_lo serves -w and line bookkeeping).  Offsets written are
 * (offset within d_text) + global_base.  d_positions may be NULL (count only) and receives at most
 * `position_capacity` records, in the reference's emission order.  `stream` is a hipStream_t (NULL =
 * default stream); with time_it != 0 the kernels are bracketed by hipEvents on that stream and the
 * call synchronises.  The kernels move 16 bytes per lane from d_text + a multiple of 16: a 16-byte aligned d_text (any
 * hipMalloc block) is the fast case; a slice at an odd offset is scanned correctly (gfx950 serves unaligned vector loads;
 * tests/test_gpu_fullsize.py scans such slices), an aligned block plus an ownership window is the better way to say it.
 * Reads: d_text is never written, and no byte outside [0, text_len) can influence a result; the list-based -c of the
 * multi-pattern scan reads whole ALIGNED 16-byte granules and so may touch up to 15 bytes behind text_len inside the granule
 * that holds the last byte (the same page: safe for any allocation, worth knowing for a slice that ends an allocation).
 * Placement: WHERE the driver puts a large allocation moves a 32-GiB read stream by 2-3 % and a scan that also writes GBs of
 * records by ~10 % (two modes, one per allocation) — the library takes the buffers as the caller made them;
 * krep_gpu_alloc_placed() below makes them with the placement drawn for.
 * Returns 0 on success, non-zero on error (krep_gpu_last_error()). */
int krep_gpu_scan_device(krep_gpu_plan_t *plan, const void *d_text, size_t text_len, size_t own_lo,
                         size_t own_hi, size_t global_base, match_position_t *d_positions,
                         uint64_t position_capacity, void *stream, int time_it,
                         krep_gpu_scan_out_t *out);

/* Device memory for a text and the records of its scans whose PLACEMENT has been drawn for (kg_place.hip).  Allocates up to `tries`
 * (1..8) candidate blocks of text_bytes (+ 64 bytes of slack) followed by record_bytes on `device`, times the single-byte workload of
 * BASELINE config 3 on each (the generator's 1 %-density text in the candidate's text area; counting only, and with the records written
 * into the candidate's record area), keeps the candidate whose record-writing scan ran fastest — the first one that runs within 1.32x of
 * its own counting scan is taken at once — and frees the others.  *d_text receives the block (hipMalloc alignment), *d_records (may be NULL
 * when record_bytes == 0) the record area inside the same block, 256-byte aligned; `info` (may be NULL) what was drawn.  The text area
 * comes back holding the probe's bytes.  tries <= 1, a text of less than 1 GiB or a record area of less than 16 bytes per 64 bytes of the
 * first GiB: one plain allocation, nothing timed.  Cost per draw at 32 GiB + 8 GiB: the allocation + ~50 ms of probe scans.
 * Free with krep_gpu_free_placed(device, *d_text).  Returns 0, or 2 (krep_gpu_last_error()). */
typedef struct krep_gpu_placement
{
    uint32_t tries;          /* candidates drawn                                  */
    uint32_t kept;           /* index of the one returned                         */
    float count_only_ms[8];  /* per draw: kernel time of the counting scan        */
    float records_ms[8];     /* per draw: median of three record-writing scans    */
} krep_gpu_placement_t;
int krep_gpu_alloc_placed(int device, size_t text_bytes, size_t record_bytes, int tries, void **d_text, void **d_records,
                          krep_gpu_placement_t *info);
int krep_gpu_free_placed(int device, void *d_text);

/* The same for a device buffer that is a SLICE [global_base, global_base + text_len) of a text of global_len bytes
 * (global_len == 0: the buffer ends the text).  The reference functions place some of their behaviour by the length of
 * the WHOLE text (the block simd_avx512_search leaves unexamined, krep.c:5171; the first byte of the scalar tail calls,
 * which has no left neighbour for -w, krep.c:5059-5097): with global_len those land where the reference puts them, in
 * whichever shard holds them.  The sequential match-set families (greedy SSE4.2/KMP selection of a bordered pattern,
 * -o through BMH / memchr_short; -c through the AVX-512 / AVX2 -w / NEON block loops) accept a window inside the text only
 * through krep_gpu_scan_device_seq() below; krep_gpu_split_mode() names the few classes that need the whole text in one window. */
int krep_gpu_scan_device_ex(krep_gpu_plan_t *plan, const void *d_text, size_t text_len, size_t own_lo,
                            size_t own_hi, size_t global_base, size_t global_len, match_position_t *d_positions,
                            uint64_t position_capacity, void *stream, int time_it, krep_gpu_scan_out_t *out);

/* ---- the sequential match-set families in pieces ("one boundary record per shard ... one exchange step") ----
 * The greedy left-to-right selection of simd_sse42_search / kmp_search (krep.c:4839-4848, :1741), boyer_moore_search under
 * -o (:1371) and memchr_short_search's -o walk (:4495) couple a match to the one before it; across a cut of the text the
 * whole coupling is ONE number: where the reference's scan stands when it enters the right-hand piece. */
typedef struct krep_gpu_seq_carry
{
    uint64_t resume;      /* greedy / -o walks: global offset from which the reference's scan continues — starts in front of
                             it are consumed, the first occurrence / candidate at or behind it is looked at afresh (0: nothing
                             consumed)                                                                                      */
    /* -c through simd_avx512_search / simd_avx2_search -w / neon_search (krep.c:5203-5218, :5000-5013, :4590-4611): the line-skip history that decides
     * where the block grid stands when it enters the last 256 bytes of the text (the end-of-text replay, kg_replay.h).
     * All offsets are global and stored + 1 (0 = none).                                                                    */
    uint64_t q1;          /* start of the last accepted occurrence in the text so far                                        */
    uint64_t nl1;         /* first '\n' at or behind it                                                                      */
    uint64_t local_q1;    /* the same for THIS piece alone: a caller that scanned its pieces out of order (shards on       */
    uint64_t local_nl1;   /* different devices) folds them afterwards: q1 = local_q1 ? local_q1 : in.q1,                   */
    uint64_t local_first_nl1; /* nl1 = local_q1 ? local_nl1 : in.nl1 ? in.nl1 : in.q1 ? local_first_nl1 : 0                 */
    /* neon_search only (krep.c:4590-4611: no restart on an unterminated line, so its block grid is still the one the previous
     * counted line set): g0 = the grid origin in effect for q's line — (first '\n' behind the last accepted occurrence on an
     * EARLIER line) + 1, or 0.  local_g0_kind: 0 no occurrence in this piece; 1 g0 = local_g0; 2 q's line starts in this piece
     * but the earlier occurrence lies in front of it: g0 = in.q1 ? (in.nl1 ? in.nl1 : local_first_nl1) : 0; 3 q's line started
     * in front of this piece: g0 = in.q1 ? (in.nl1 ? in.nl1 : in.g0) : 0.                                                    */
    uint64_t g0, local_g0, local_g0_kind;
    /* -c with a '\n' inside a pattern.  Multi-pattern (aho_corasick.c:383-396: the counter is bumped whenever the line of a match
     * START differs from the line of the previously counted one, matches visited in emission order — end ascending): a piece
     * owns the matches that END in it, its list continues its predecessor's, and the coupling is two numbers.  Through
     * simd_sse42_search / kmp_search (krep.c:4785-4795, :1703-1707): a piece owns the occurrences that START in it; the
     * coupling is `resume` above (where the reference's scan stands) plus the same two numbers:                           */
    uint64_t nl_before;   /* '\n' bytes of the text in front of this piece's own_hi (carry_out) / own_lo (carry_in)         */
    uint64_t last_line;   /* 1-based line number of the START of the last match of the text so far (0: no match yet)        */
    uint64_t local_nl;    /* this piece alone: '\n' bytes in [own_lo, own_hi) ...                                           */
    uint64_t local_last;  /* ... and the line of its last match's start RELATIVE to own_lo, biased by 2^62 (0: no match):   */
                          /* a caller folding out-of-order pieces: nl_before = in.nl_before + local_nl,                      */
                          /* last_line = local_last ? in.nl_before + 1 + (local_last - 2^62) : in.last_line                  */
    uint64_t local_lines; /* -c through the block loops, the piece that ENDS the text: its canonical line count in front of the   */
                          /* end-of-text replay, stored + 1 (0: not that piece) — what krep_gpu_replay_tail() starts from         */
} krep_gpu_seq_carry_t;
/* krep_gpu_scan_device_ex() for the pieces of one text IN TEXT ORDER: carry_in = the record the previous piece left
 * (NULL: nothing in front of this window is consumed — the piece that starts the text, or an optimistic first pass of a
 * shard whose left neighbour is still running: compare its assumption with the neighbour's carry_out afterwards and re-run
 * the piece if they differ), carry_out (nullable) = this piece's record.  Families without a sequential dependency pass
 * the record through unchanged.  For the -c block-loop family only the piece that ENDS the text depends on the record (it
 * must be at least 4 KiB long); the others only extend it. */
int krep_gpu_scan_device_seq(krep_gpu_plan_t *plan, const void *d_text, size_t text_len, size_t own_lo, size_t own_hi,
                             size_t global_base, size_t global_len, match_position_t *d_positions, uint64_t position_capacity,
                             void *stream, int time_it, const krep_gpu_seq_carry_t *carry_in, krep_gpu_seq_carry_t *carry_out,
                             krep_gpu_scan_out_t *out);
/* The end-of-text replay ALONE (-c through the block loops).  The piece that ends the text was scanned with a guessed record
 * (its shard started before its left neighbours had finished); `carry_true` is what the text in front of it really leaves,
 * `piece` the record that piece produced (its local_* fields: its own line-skip contribution and local_lines).  d_tail holds the
 * last tail_len bytes of the text (at least 512, or the whole text) — nothing else of the piece is read again.  Returns in
 * *lines what krep_gpu_scan_device_seq() would have reported as line_count / count for that piece had it been given carry_true,
 * and in *carry_out the record it would have left.  (the multi-shard operators re-staged and re-scanned that piece.) */
int krep_gpu_replay_tail(krep_gpu_plan_t *plan, const void *d_tail, size_t tail_len, size_t global_len, void *stream,
                         const krep_gpu_seq_carry_t *carry_true, const krep_gpu_seq_carry_t *piece, krep_gpu_seq_carry_t *carry_out,
                         uint64_t *lines);
/* How a text of text_len bytes may be cut for `params` under the current configuration. */
enum krep_gpu_split
{
    KREP_GPU_SPLIT_WHOLE = 0,  /* one window only: neon_search's max_count == 0 corner, -c with -o through
                                  memchr_short_search (never produced by krep's main()), and a regex that can overlap
                                  itself without -c (krep_gpu_regex_compile; an alternation: cross_overlap)                */
    KREP_GPU_SPLIT_PIECES = 1, /* independent pieces: start-offset ownership + halo, results concatenate / merge          */
    KREP_GPU_SPLIT_CHAIN = 2   /* pieces in text order through krep_gpu_scan_device_seq() (round 5: also -c with a newline
                                  inside a pattern, multi-pattern and through simd_sse42_search / kmp_search)             */
};
int krep_gpu_split_mode(const search_params_t *params, size_t text_len);

/* Deterministic synthetic haystacks, generated directly in HBM by a counter-based
 * PRNG so that any [global_off, global_off+len) slice is reproducible on any rank.
 * kind: 2 = background a-z/space/newline + planted 8-byte literal every `period` bytes (cfg 2/5),
 *       3 = background + target byte with probability 1/100 (cfg 3),
 *       4 = background + planted dictionary words (cfg 4; `plant`/`plant_len` = packed patterns),
 *       5 = word text: `period`-byte lines ('\n'-terminated) of words drawn from the packed list `plant` with p(rank) ~ 1/rank,
 *           single blanks between them (the natural-language-like text of cfg 1 / the reference's own benchmark corpus). */
int krep_gpu_generate(void *d_dst, size_t len, size_t global_off, int kind, uint64_t seed,
                      const void *plant, size_t plant_len, uint64_t period, void *stream);
/* Host twin of the generator (same bytes), for parity tests and the CPU baseline. */
void krep_gpu_generate_host(void *dst, size_t len, size_t global_off, int kind, uint64_t seed,
                            const void *plant, size_t plant_len, uint64_t period);

/* Combine per-shard line bookkeeping left-to-right (the one "exchange step" of the multi-GPU path):
 * returns the global distinct-line count given shard outputs in shard order. */
uint64_t krep_gpu_combine_line_counts(const krep_gpu_scan_out_t *shards, int n);

/* ---- the collective of the multi-GPU path: per-shard counters meet in ONE RCCL all-reduce over xGMI -------
 * One process driving several devices (search_buffer(num_gpus > 1), the operators with cfg.num_gpus > 1) does this
 * internally (ncclCommInitAll over the devices used).  One process PER GPU (bench.py under torch.distributed.run) uses the
 * rank-level calls below: rank 0 draws an id, the host program's own bootstrap carries its 128 bytes to the other ranks,
 * every rank joins, and each scan ends with one all-reduce of its counters {matches, lines, ...}.  librccl is opened on
 * first use (dlopen); all return 0, or 2 with krep_gpu_last_error() set. */
#define KREP_GPU_COMM_ID_BYTES 128
int krep_gpu_comm_unique_id(void *id128);
int krep_gpu_comm_init_rank(const void *id128, int nranks, int rank, int device);
int krep_gpu_comm_allreduce_u64(uint64_t *values, int n);                         /* host values, in place; synchronous  */
int krep_gpu_comm_allreduce_device_u64(void *d_values, int n, void *stream);      /* device-resident, in place, async    */
void krep_gpu_comm_destroy(void);
uint64_t krep_gpu_rccl_calls(void); /* collectives this process has issued through RCCL (diagnostic / self-test) */
int krep_gpu_rccl_version(void);    /* ncclGetVersion(), 0 when librccl cannot be loaded */
/* Where the calling thread's LAST sharded host search (search_buffer(num_gpus > 1), the operators with num_gpus > 1) ran:
 * logical shards, the distinct physical devices they were placed on, the ranks of the communicator the counters met in
 * (0: a single device, nothing to reduce) and how they met (1 = the RCCL all-reduce, 2 = RCCL could not be used and the
 * host summed the slots it already held — the search result is the same, krep_gpu_last_error() names the reason).
 * The multi-GPU self-test (tests/test_gpu_multi.py) asserts on it; a search that did not shard leaves shards = 1. */
typedef struct krep_gpu_shard_info
{
    int shards;          /* logical shards of the text                                  */
    int devices_used;    /* distinct physical devices                                   */
    int device_ids[16];  /* the first 16 of them, in shard order                        */
    int comm_ranks;      /* ranks of the communicator (ncclCommInitAll over the devices) */
    int reduced_by;      /* 0 nothing to reduce, 1 RCCL, 2 host sum after an RCCL failure */
} krep_gpu_shard_info_t;
void krep_gpu_last_shard_info(krep_gpu_shard_info_t *out);

/* ---- formatter-side post-processing in HBM (what search_file() does on one host thread after the scan) --------------
 * krep_gpu_order_by_start: the (start, end) order of compare_match_positions (krep.c:420-434) that search_file()
 *   establishes with qsort() before printing (krep.c:3018-3023).  Input: n records ascending in `end` (the order of
 *   every operator of this library); one stable device radix sort keyed on `start`, in place.
 * krep_gpu_line_numbers: the 1-based line number of every record's start, as print_matching_items() derives them by
 *   counting newlines (krep.c:589-668); d_lines[n] on the device.
 * krep_gpu_set_result_order(1): krep_gpu_aho_corasick_search() hands back its records already in (start, end) order
 *   (sorted on the device before the copy to the host), so the caller may skip its qsort().  Default 0: the
 *   reference's emission order (end ascending, longest first).
 * All return 0, or 2 with krep_gpu_last_error() set. */
/* max_offset: upper bound of every start offset in the list (the WHOLE text's length when the records carry a
 * global_base) — the radix key is sized from it.  Limit: n <= 2^31 - 1 records (34 GB of match_position_t; the device
 * radix sort counts its items in an int) — a longer list is refused with an error, never truncated. */
int krep_gpu_order_by_start(match_position_t *d_positions, uint64_t n, size_t max_offset, void *stream);
/* records must be relative to d_text[0]; use the _ex form (records minus global_base) for shard lists.  A record outside
 * [global_base, global_base + text_len] gets line number 0. */
int krep_gpu_line_numbers(const void *d_text, size_t text_len, const match_position_t *d_positions, uint64_t n,
                          uint64_t *d_lines, void *stream);
int krep_gpu_line_numbers_ex(const void *d_text, size_t text_len, size_t global_base, const match_position_t *d_positions,
                             uint64_t n, uint64_t *d_lines, void *stream);
void krep_gpu_set_result_order(int by_start);

/* ---- the matching lines of a text in HBM: the reference's default output (print_matching_items(), full-line mode without colour,
 * krep.c:797-1071) ----
 * Input: the whole text in one buffer and its n records in (start, end) order, relative to d_text[0] (krep_gpu_order_by_start()
 * on a multi-pattern list; a single literal's list is in that order already).  A record belongs to the line of its START:
 * line_start = one past the last '\n' in [0, start), line_end = the first '\n' at or after it, else text_len.  Each distinct line
 * once, ascending, at most max_lines of them (SIZE_MAX: all, 0: none).  Only the first 2048 records of a line take part in its
 * bytes (MAX_MATCHES_PER_LINE; the reference warns on stderr: capped_lines).  A line's bytes follow the reference's cursor, which
 * starts at line_start: per record text[cursor, start) if start > cursor, then the match clamped to line_end, and the cursor
 * moves to the clamped end, also backwards — overlapping or nested records repeat bytes ("xx Sherlock yy" with the records of
 * Sherlock, er and lock prints "xx Sherlockerlock yy"); then text[cursor, line_end) and '\n'.  A record whose clamped match is
 * empty (end == start, or a start ON a '\n', where the reference CLI does not terminate) adds nothing of its own.
 * A list that is not ascending in start, or holds a record with start >= text_len or end < start, is refused (2) before any
 * byte of the text is read through it.  These calls take the WHOLE text; a text in pieces (a shard, a streamed buffer: a line may
 * cross a cut) goes through krep_gpu_format_lines_window below.  The strings of a coloured output go in through
 * krep_gpu_format_lines_ex below.
 * The calls return 0, or 2 with krep_gpu_last_error() set, and synchronise `stream` before they return.  A NULL output pointer
 * or a capacity of 0 is a size query.  A capacity that is too small sets `overflow` and returns 0: the sizes are valid, the
 * output buffers hold nothing usable. */
typedef struct krep_gpu_lines_out
{
    uint64_t lines;        /* distinct lines emitted (after max_lines)                                   */
    uint64_t lines_total;  /* distinct lines that hold a record's start                                  */
    uint64_t out_bytes;    /* bytes krep_gpu_format_lines wrote, or needs (0 from krep_gpu_matching_lines) */
    uint64_t capped_lines; /* emitted lines with more than 2048 records                                  */
    int overflow;          /* a capacity was too small                                                   */
} krep_gpu_lines_out_t;
/* d_lines[l] = {line_start, line_end} of the l-th emitted line; d_first_record[l] = index of its first record, and
 * d_first_record[lines] = index one past the records of the last emitted line (ALL its records, not only the first 2048): it
 * holds line_capacity + 1 entries. */
int krep_gpu_matching_lines(const void *d_text, size_t text_len, const match_position_t *d_positions, uint64_t n,
                            uint64_t max_lines, match_position_t *d_lines, uint64_t *d_first_record, uint64_t line_capacity,
                            krep_gpu_lines_out_t *out, void *stream);
/* the bytes themselves into d_out (device memory, any alignment); prefix = "FILE:" in front of every line, or empty (a host string) */
int krep_gpu_format_lines(const void *d_text, size_t text_len, const match_position_t *d_positions, uint64_t n,
                          uint64_t max_lines, const char *prefix, size_t prefix_len, void *d_out, size_t out_capacity,
                          krep_gpu_lines_out_t *out, void *stream);
/* The same lines with the caller's strings in them: what the reference prints under --color=always (krep.c:797-1071 with
 * color_output_enabled).  Per emitted line:
 *     prefix
 *     per counted record (the first 2048 of the line) whose match, clamped to line_end, is not empty:
 *         text[cursor, start) if start > cursor,  before_match,  text[start, clamped end),  after_match;  cursor = clamped end
 *     text[cursor, line_end) if cursor < line_end,  line_close,  '\n'
 * A record whose clamped match is empty adds nothing, no strings either; overlapping records repeat bytes, each inside its own
 * pair of strings.  The strings are the caller's, the library knows no escape code: the reference uses prefix = filename colour,
 * FILE, reset, separator colour, ":", text colour (the text colour alone without a filename), before_match = match colour,
 * after_match = text colour, line_close = reset (krep.h:34-39).  With only `prefix` set the bytes are those of
 * krep_gpu_format_lines.  Everything else is as for krep_gpu_format_lines: the record order, the refusal (2) of a list that is
 * not ascending or out of range before the text is read, the size query, `overflow` with valid sizes, any alignment of d_text
 * and d_out, nothing written outside [d_out, d_out + out_bytes), `stream` synchronised, n == 0 leaves everything 0.  A string
 * of more than 2^20 bytes is refused (2). */
typedef struct krep_gpu_line_format /* host strings, each may be NULL with length 0 */
{
    const char *prefix;
    size_t prefix_len;
    const char *before_match;
    size_t before_match_len;
    const char *after_match;
    size_t after_match_len;
    const char *line_close;
    size_t line_close_len;
} krep_gpu_line_format_t;
int krep_gpu_format_lines_ex(const void *d_text, size_t text_len, const match_position_t *d_positions, uint64_t n,
                             uint64_t max_lines, const krep_gpu_line_format_t *fmt /* NULL: all empty */, void *d_out,
                             size_t out_capacity, krep_gpu_lines_out_t *out, void *stream);

/* ---- the same lines for a text in pieces: one call per WINDOW, the outputs concatenate ----
 * The window contract of the scans (start ownership + halo) for the line output.  `fmt`, the bytes of an emitted line, the cursor
 * rule, the clamp to line_end, the 2048-records-per-line cap and capped_lines, "an empty clamped match adds nothing" and "at most
 * max_lines lines" are those of krep_gpu_format_lines_ex.
 * Buffer: d_text[0 .. text_len) holds text[global_base .. global_base + text_len); it ends the text when global_base + text_len ==
 *   global_len.
 * Records: GLOBAL offsets, as krep_gpu_scan_device_ex writes them with a global_base, in (start, end) order.  A list that is not
 *   ascending in start, or holds a record with start outside [global_base, global_base + text_len) or end < start, is refused (2)
 *   before any byte of the text is read through it: the rule of the whole-text calls.
 * Line start: one past the last '\n' in [global_base, start).  With no such newline it is 0 when global_base == 0; otherwise the
 *   line starts in front of the buffer, is not owned, and the record is passed over silently.
 * Ownership: the call owns the lines with line_start in [own_lo, own_hi); records of other lines are passed over, they are a
 *   neighbour's.  So the ONE byte in front of own_lo is all the left context a window needs.  A record that starts ON a '\n'
 *   belongs to the line that newline ends.
 * Line end: the first '\n' at or after line_start inside the buffer.  An owned matching line is COMPLETE when that newline exists and
 *   lies in front of records_hi (the list holds every record with start < records_hi, so all of the line's); or when the buffer ends
 *   the text and records_hi == global_len: then line_end = global_len serves a last line without a newline.  Otherwise the line is
 *   incomplete — at most one can be, the last owned one.  It is not emitted and not counted in lines / lines_total.  If it would have
 *   been emitted (its index among the owned matching lines is < max_lines) it is reported: incomplete_line_start1 = its global
 *   line_start + 1, incomplete_first_record = the index of its first record.  The caller submits it again as a window of its own
 *   (own_lo = line_start, own_hi = line_start + 1) with a longer buffer.
 *   What the call cannot see: an owned line that outruns the buffer and whose FIRST record lies at or behind records_hi (no record
 *   of it is in the list).  That can only be the line that is open at records_hi; a caller that cuts its halos short looks for it.
 * Window: global_base <= own_lo <= own_hi <= records_hi <= global_base + text_len <= global_len, and own_lo > global_base unless
 *   both are 0; anything else is refused (2).
 * Invariant: cut a text at 0 = c0 < c1 < ... < ck = global_len, give window [ci, ci+1) a buffer from ci - 1 (or 0) far enough to the
 *   right that nothing is incomplete, state records_hi truthfully and pass max_lines on as what is left: the outputs, concatenated,
 *   are the bytes of krep_gpu_format_lines_ex on the whole text, and lines, lines_total and capped_lines sum to its values.
 * -m: cutting the record list to its first max_count records in EMISSION order is a property of the whole list; it stays with the
 *   caller, as it does for the whole-text calls.
 * As for krep_gpu_format_lines_ex: d_out == NULL or out_capacity == 0 is a size query, `overflow` comes with valid sizes, d_text and
 *   d_out may have any alignment, nothing is written outside [d_out, d_out + out_bytes), `stream` is synchronised on return, a
 *   string of more than 2^20 bytes and n >= 2^40 are refused (2), n == 0 leaves everything 0 (after the window has been checked). */
typedef struct krep_gpu_lines_window
{
    size_t global_base;    /* offset in the text of d_text[0]                                                      */
    size_t global_len;     /* length of the whole text                                                             */
    size_t own_lo, own_hi; /* global offsets: the call owns the lines whose line_start is in [own_lo, own_hi)      */
    size_t records_hi;     /* the record list is complete for every start < records_hi (global)                    */
} krep_gpu_lines_window_t;
typedef struct krep_gpu_lines_window_out
{
    krep_gpu_lines_out_t lines;       /* lines, lines_total, out_bytes, capped_lines, overflow: of the OWNED, COMPLETE lines */
    uint64_t incomplete_line_start1;  /* global line_start + 1 of the owned matching line that could not be completed (0: none) */
    uint64_t incomplete_first_record; /* index of its first record in the list (n when none)                                    */
} krep_gpu_lines_window_out_t;
int krep_gpu_format_lines_window(const void *d_text, size_t text_len, const krep_gpu_lines_window_t *win,
                                 const match_position_t *d_positions, uint64_t n, uint64_t max_lines,
                                 const krep_gpu_line_format_t *fmt /* NULL: all empty */, void *d_out, size_t out_capacity,
                                 krep_gpu_lines_window_out_t *out, void *stream);

/* ---- the matches of a text in HBM, one per line: the reference's -o output (print_matching_items(), only-matching mode,
 * krep.c:517-793) ----
 * Input as for the whole-text line calls: the whole text (a text in pieces goes through krep_gpu_format_matches_window below) and its n
 * records in (start, end) order, n being the reference's result->count (search_file() has
 * cut the list to its first max_count records in emission order and ordered it).  For record i < min(n, max_items), in list order:
 *     prefix  before_number  LINE ':'  after_number  MATCH  after_match  '\n'
 * The four strings are the caller's ("FILE:" and nothing else without colour; the escape codes of krep.h:34-39 with it: the library
 * knows none).  MATCH is text[start, min(end, text_len)) with every '\n' inside it replaced by a blank (krep.c:736-747).
 * LINE is the 1-based line of the record's start (a start ON a '\n' belongs to the line that newline ends), with the reference's
 * exception: once a list holds more than 10 records the reference looks the line up in an index of the text's newlines
 * (krep.c:531-556, :619-653), and a record that starts behind the text's LAST newline finds no entry there and prints the number of
 * the search before it: LINE of the nearest earlier record that starts at or before the last newline, or 1 when there is none.  A
 * list of at most 10 records, or a text without a newline, prints true numbers throughout.
 * A list that is not ascending in start, or holds a record with start >= text_len or end < start, is refused (2) before any byte of
 * the text is read through it (the reference passes over such a record; the calls above refuse the list, and so does this one).
 * A match longer than the reference's 8 MiB batch buffer is outside what its code defines; here it is copied like any other.
 * Returns 0, or 2 with krep_gpu_last_error() set (a string of more than 2^20 bytes, n >= 2^40, a failing HIP call), and synchronises
 * `stream` before it returns.  d_out == NULL or out_capacity == 0 is a size query; a capacity that is too small sets `overflow` and
 * returns 0 with valid sizes and nothing usable in d_out.  d_text and d_out may have any alignment; nothing is written outside
 * [d_out, d_out + out_bytes).  n == 0 leaves everything 0. */
typedef struct krep_gpu_match_format /* host strings, each may be NULL with length 0 */
{
    const char *prefix;
    size_t prefix_len;
    const char *before_number;
    size_t before_number_len;
    const char *after_number;
    size_t after_number_len;
    const char *after_match;
    size_t after_match_len;
} krep_gpu_match_format_t;
typedef struct krep_gpu_matches_out
{
    uint64_t items;     /* records emitted = min(n, max_items) */
    uint64_t out_bytes; /* bytes written, or needed            */
    int overflow;       /* out_capacity was too small          */
} krep_gpu_matches_out_t;
int krep_gpu_format_matches(const void *d_text, size_t text_len, const match_position_t *d_positions, uint64_t n,
                            uint64_t max_items, const krep_gpu_match_format_t *fmt /* NULL: all empty */, void *d_out,
                            size_t out_capacity, krep_gpu_matches_out_t *out, void *stream);

/* ---- the same -o output for a text in pieces: one call per WINDOW, the outputs concatenate ----
 * `fmt`, the bytes of a record (prefix before_number LINE ':' after_number MATCH after_match '\n', every '\n' inside MATCH a blank, an
 * empty match an empty MATCH) and "at most max_items records" are those of krep_gpu_format_matches.
 * Buffer: d_text[0 .. text_len) holds text[global_base .. global_base + text_len); it ends the text when global_base + text_len ==
 *   global_len.
 * Records: GLOBAL offsets, as krep_gpu_scan_device_ex / _seq write them with a global_base, in (start, end) order; the list is any
 *   consecutive run of the whole text's list.  Ownership is the scan's: the call emits every record it is given (a record is one
 *   item and belongs to whoever scanned it), so there is no own_lo / own_hi.  MATCH is text[start, min(end, global_len)).
 *   Refused (2) before any byte of the text is read through the list: a list not ascending in start, a record with start outside
 *   [global_base, global_base + text_len) or end < start, or a match that outruns the buffer (min(end, global_len) > global_base +
 *   text_len: a match is no longer than the longest match of the search -- the longest pattern of a literal search, L / Lmax of the
 *   regex compilers under -E, where `a{16}` is five pattern bytes and sixteen text bytes -- so the caller can always size its halo;
 *   nothing is "incomplete").
 * LINE: the true number is 1 + newlines_before + the newlines in d_text[0, start - global_base); a start ON a '\n' belongs to the line
 *   that newline ends.  The reference's stale number (above) applies when stale_rule != 0, last_newline1 != 0 and start >=
 *   last_newline1 — decided by OFFSET, the window does not know the text's newline total.  Such a record prints S: the largest true
 *   LINE among this list's n records (all n, not only the emitted ones) with start < last_newline1; win->stale_line when the list
 *   has none; 1 when that is 0 too.
 * Carries out, valid for n == 0 too (a window without records still advances the line count), on a size query and with overflow:
 *   out->stale_line = S before the fallback to 1 (the largest such LINE of this list, else win->stale_line);
 *   out->newlines_before_count_to = newlines_before + the newlines in d_text[0, count_to - global_base).
 * Also refused (2): global_base + text_len > global_len, count_to outside [global_base, global_base + text_len], last_newline1 >
 *   global_len, global_len >= 10^16 or a LINE of more than 16 digits, a format string of more than 2^20 bytes, n >= 2^40, NULL win / out.
 * Invariant: cut the whole list into consecutive sub-lists in order; give each a buffer that holds its records, with non-decreasing
 *   global_base; set count_to to the next buffer's global_base; chain newlines_before (<- newlines_before_count_to) and stale_line;
 *   give every call the same truthful last_newline1 and stale_rule; pass max_items on as what is left.  The outputs, concatenated, are
 *   byte for byte those of krep_gpu_format_matches on the whole text, and `items` sums to its value.
 * As for krep_gpu_format_matches: d_out == NULL or out_capacity == 0 is a size query, `overflow` comes with valid sizes, d_text and d_out
 *   may have any alignment, nothing is written outside [d_out, d_out + out_bytes), `stream` is synchronised on return. */
typedef struct krep_gpu_matches_window
{
    size_t global_base;       /* offset in the text of d_text[0]                                                                 */
    size_t global_len;        /* length of the whole text                                                                        */
    size_t count_to;          /* global offset in [global_base, global_base + text_len]: see newlines_before_count_to            */
    uint64_t newlines_before; /* '\n' bytes in text[0, global_base)                                                              */
    uint64_t last_newline1;   /* global offset of the text's LAST '\n', + 1 (0: the text has none)                               */
    uint64_t stale_line;      /* LINE of the nearest record IN FRONT of this list that starts at or before the last newline (0:
                                 none)                                                                                           */
    int stale_rule;           /* the whole list of the text, after its max_count cut, holds more than 10 records                 */
    int reserved;             /* (keeps the size free of implicit padding; not read)                                             */
} krep_gpu_matches_window_t;
typedef struct krep_gpu_matches_window_out
{
    krep_gpu_matches_out_t matches;    /* items, out_bytes, overflow: of the records of this call                                */
    uint64_t newlines_before_count_to; /* '\n' bytes in text[0, count_to): the next window's newlines_before                     */
    uint64_t stale_line;               /* the next window's stale_line                                                           */
} krep_gpu_matches_window_out_t;
int krep_gpu_format_matches_window(const void *d_text, size_t text_len, const krep_gpu_matches_window_t *win,
                                   const match_position_t *d_positions, uint64_t n, uint64_t max_items,
                                   const krep_gpu_match_format_t *fmt /* NULL: all empty */, void *d_out, size_t out_capacity,
                                   krep_gpu_matches_window_out_t *out, void *stream);

/* ---- a batch of texts in one scan: krep -r (search_directory_recursive() -> search_file() once per file, krep.c) ----
 * One operator call costs 50-80 us of launch and synchronisation plus staging, so a tree of ten thousand files of 4-200 KiB never
 * reaches the device one file at a time (min_text_bytes above).  A batch makes many texts ONE text: the items are packed into one
 * device buffer with exactly one '\n' between neighbours (none in front of the first, none behind the last), the pack is scanned
 * once with records, and the record list is cut back into per-item results on the device (krep_amd/csrc/kg_batch.hip).
 * Contract: for every item i, results[i].count and the records [first_record, first_record + n_records) of `records` are what the
 *   operator krep_gpu_select_search_algorithm(params) returns produces for (items[i].text, items[i].len) ALONE — the same count, every
 *   (start, end) relative to the item's own first byte, the reference's emission order inside an item; items appear in `records`
 *   in item order.  An item of length 0 has count 0.  n_records is 0 when positions are not tracked (track_positions == false,
 *   or count_lines_mode: the pack is scanned with records and an item's count is the number of distinct lines that hold one of its
 *   record starts; the records themselves are not returned).
 * When that is exact: a search is batchable iff its result is newline-separable — for all texts A and B, result(A + '\n' + B) =
 *   result(A) followed by result(B) shifted by |A| + 1 (under -c: count(A + '\n' + B) = count(A) + count(B)).  That holds when no
 *   match can contain '\n' (matches neither cross the separator nor couple across it: the greedy and -o selections included), -w
 *   sees a non-word byte at both item edges ('\n' is one), and the reference function behaves the same wherever a line stands in
 *   the text.  krep_gpu_batch_can_accelerate() is 1 iff krep_gpu_can_accelerate(params) is 1 and none of these holds (each has its
 *   own reason in krep_gpu_last_error()):
 *   - a literal pattern holds '\n';
 *   - under -E a byte class of the compiled program holds '\n' ([[:space:]], [^a] never does in glibc's C locale: REG_NEWLINE);
 *     ^ and $ are fine (the separator is a real newline, the first and last item sit at the true text edges) — except $ with
 *     case_sensitive == false: the REG_NOTEOL quirk (the end of the text ends no line) applies at the end of EVERY item alone and
 *     in the pack only at the end of the last;
 *   - the reference function places behaviour by absolute position or by the whole text's length (what krep_gpu_scan_device_ex()
 *     needs global_len for, and what krep_gpu_split_mode() calls WHOLE): -c through the block loops of simd_avx512_search,
 *     simd_avx2_search with -w and neon_search (the end-of-text replay); simd_avx512_search without -c (the block it leaves
 *     unexamined at the text's end); -w through the scalar tail of simd_avx2_search / simd_avx512_search / neon_search (its first
 *     byte has no left neighbour); neon_search with max_count == 0; -c with -o through memchr_short_search.  A regex plan that is
 *     WHOLE is NOT refused for that alone: its overlap never crosses a newline and the pack is scanned in one window;
 *   - memchr_short_search under -o with a 3-byte pattern: its walk skips pattern_len bytes behind a FAILED candidate too
 *     (krep.c:4495), so a candidate on the last byte of an item steps over the first byte of the next one — alone, the item ends
 *     the walk there;
 *   - -o through simd_avx2_search / neon_search with a pattern that can overlap itself: the block body reports every occurrence,
 *     the scalar tail is boyer_moore_search, which under -o skips a match's length (krep.c:1371), and where that tail begins
 *     depends on the whole text's length;
 *   - max_count != SIZE_MAX: the per-function max_count quirks are a property of each item's own list; cutting per item is
 *     follow-up work.  (That is the answer while the switch below is off, which it is by default.)
 * max_count behind a switch.  krep_gpu_set_batch_max_count(1) — process-wide, off unless $KREP_GPU_BATCH_MAX_COUNT=1 is set when the
 *   library is loaded — makes a finite max_count no reason to refuse: krep_gpu_batch_can_accelerate(), krep_gpu_search_batch() and
 *   krep_gpu_grep_batch() then take it, and every other refusal above stands with its own text.  Two max_count == 0 corners are placed
 *   by the position in the text and stay refused, each with a reason of its own: neon_search (above), and a count-only search
 *   through simd_avx2_search (a hit in the block body answers 1, a hit in the scalar tail is capped back to 0, krep.c:5036, :5066-5093).  Off, all three behave and report as if the switch did not exist.  The pack is still scanned
 *   without a limit; each item's list is cut on the device, and the contract above holds with params as given: per item, what the
 *   operator produces for the item ALONE under that max_count.  With T the item's records in the unlimited list R (emission order),
 *   Ln its distinct lines and M = max_count:
 *   - count = min(Ln, M) under count_lines_mode, else min(T, M).  M == 0 gives 0, except that a count-only search (neither
 *     track_positions nor count_lines_mode) through boyer_moore_search, memchr_short_search or a regex gives T > 0 ? 1 : 0
 *     (krep.c:1355-1367);
 *   - records (where the batch returns records at all): the first min(T, M) of R; through kmp_search one more when T > M
 *     (krep.c:1717-1724); through memchr_search, when T > M, M > 0 and M % 4096 == 0, the flush displacement (krep.c:3976-3991):
 *     R[0 .. M-4096), R[M], R[M-4096 .. M-1) — M records, R[M-1] dropped; M == 0 keeps nothing; a multi-pattern list is cut in
 *     emission order (end ascending), not in start order;
 *   - krep_gpu_grep_batch() repeats search_file() behind the function (krep.c:2954-2981, :3018-3026): the item's list is cut to its
 *     first M records of the above (kmp_search's extra record goes), put in (start, end) order and formatted; the -o stale-number rule
 *     ("more than 10 records") sees the cut count; COUNT prints min(count, M), which is per_item[i].count too (0 in the count-only
 *     M == 0 corner, where search_file caps).
 *   info->total_records stays the number of records the scans produced — the UNCUT number; the sum of n_records is what came back.
 * Failure (a refused search, allocation, copy, launch): nothing is appended to `records`, `results` is not written, the call
 *   returns 2 and krep_gpu_last_error() names the reason.  The batch call has NO CPU fallback of its own (the selector registered
 *   with krep_gpu_set_cpu_fallback() is not asked): the caller loops over its files with its CPU function, as it does today.
 * Size: a batch whose packed size exceeds what one device buffer of the host path takes (two pieces of cfg->stream_chunk_bytes,
 *   256 MiB by default) is scanned in several packs, cut between items and never inside one; info->scans says how many.
 * items[i].text are HOST pointers; records == NULL: counts only.  cfg == NULL: the calling thread's current configuration;
 *   the pack runs on cfg->device alone (sharding a batch over several devices is follow-up work). */
typedef struct krep_gpu_batch_item
{
    const char *text; /* host pointer; may be NULL when len == 0 */
    size_t len;
} krep_gpu_batch_item_t;
typedef struct krep_gpu_batch_result
{
    uint64_t count;        /* what the reference function returns for THIS item alone (matches, or lines under count_lines_mode) */
    uint64_t first_record; /* index into records->positions of the item's first record                                          */
    uint64_t n_records;    /* its records (0 when positions are not tracked)                                                     */
} krep_gpu_batch_result_t;
typedef struct krep_gpu_batch_info
{
    uint64_t packed_bytes;  /* bytes staged: the items and the separators between them, over all packs */
    uint64_t scans;         /* packs scanned                                                           */
    uint64_t total_records; /* records the scans produced (under count_lines_mode too; under max_count: before the cut) */
    float kernel_ms;        /* hipEvent time of the scan kernels, summed over the packs                */
} krep_gpu_batch_info_t;
int krep_gpu_batch_can_accelerate(const search_params_t *params); /* 1 / 0, the reason in krep_gpu_last_error() */
void krep_gpu_set_batch_max_count(int on); /* process-wide; default 0, or $KREP_GPU_BATCH_MAX_COUNT at load */
int krep_gpu_get_batch_max_count(void);
int krep_gpu_search_batch(const search_params_t *params, const krep_gpu_config_t *cfg /* NULL: current */,
                          const krep_gpu_batch_item_t *items, size_t n_items, krep_gpu_batch_result_t *results /* n_items */,
                          match_result_t *records /* nullable */, krep_gpu_batch_info_t *info /* nullable */); /* 0, or 2 */

/* ---- the grep output of a batch: the two formatters over a PACK, and the host call that prints a batch (krep -r) ----
 * The searches a batch takes are newline-separable, so every line of a pack lies inside one item, the separator is a real newline that
 * ends an item's last line, and no record touches a separator: the whole pack is formatted in one go while it lies in HBM, and only
 * the prefix, the line-number base and the stale-number rule are looked up per item (krep_amd/csrc/kg_batch_format.hip).
 * The pack is laid out as krep_gpu_search_batch() lays it out: the items joined by one '\n', d_item_off[0 .. n_items] ascending with
 *   d_item_off[n_items] = packed_len + 1, item i = d_pack[d_item_off[i], d_item_off[i + 1] - 1).  The records carry PACK offsets and
 *   are in (start, end) order (krep_gpu_order_by_start() first on a multi-pattern list).  Item i's prefix is
 *   d_prefix_bytes[d_prefix_off[i], d_prefix_off[i + 1]); the prefixes are the caller's ("FILE:", with or without escape codes: the
 *   library knows none).  fmt->prefix must be empty (length 0), else 2.  All four pointers of the view are DEVICE pointers.
 * Contract: the output is, byte for byte, the concatenation over i = 0 .. n_items - 1 of what krep_gpu_format_lines_ex (respectively
 *   krep_gpu_format_matches) writes for the text of item i alone, item i's records rebased to the item's first byte, the same strings
 *   with prefix = prefix i, and max_lines / max_items = all.  d_item_out_off[i] (if not NULL; n_items + 1 entries) is where item i's
 *   bytes begin, entry n_items is out_bytes; an item without records adds nothing.  Per item this carries over the cursor rule, the
 *   clamp to line_end, the 2048-records-per-line cap and capped_lines, and the '\n' behind an item's last line whether or not the
 *   item ends in one; under -o, LINE restarts at 1 in every item and the reference's stale number is applied per item (it prints once
 *   per file): in an item with more than 10 records and at least one newline, a record that starts behind the item's last newline
 *   prints the LINE of the nearest earlier record of the SAME item that starts at or before that newline, or 1 when there is none.
 * Refused (2) before any byte of the pack is read through the list: a list not ascending in start; end < start; a record whose start
 *   is not inside an item (on a separator, or >= packed_len) or whose end lies behind its item's end; an offset table that is not
 *   ascending, does not begin at 0 or does not end on packed_len + 1; a prefix table that is not ascending; a string or a prefix of
 *   more than 2^20 bytes; n >= 2^40.
 * Everything else as for the single-text formatters: d_out == NULL or out_capacity == 0 is a size query (the item offsets are valid
 *   then too), a capacity that is too small sets `overflow` with valid sizes, d_pack and d_out may have any alignment, nothing is
 *   written outside [d_out, d_out + out_bytes), `stream` is synchronised on return, n == 0 leaves the sizes 0 and every item offset 0. */
typedef struct krep_gpu_pack_view /* all device pointers */
{
    const uint64_t *d_item_off;   /* [n_items + 1]                    */
    uint64_t n_items;
    const void *d_prefix_bytes;   /* the prefixes behind one another  */
    const uint64_t *d_prefix_off; /* [n_items + 1]                    */
} krep_gpu_pack_view_t;
int krep_gpu_format_lines_items(const void *d_pack, size_t packed_len, const krep_gpu_pack_view_t *v,
                                const match_position_t *d_positions, uint64_t n, const krep_gpu_line_format_t *fmt /* NULL: all empty */,
                                void *d_out, size_t out_capacity, uint64_t *d_item_out_off /* n_items + 1, nullable */,
                                krep_gpu_lines_out_t *out, void *stream);
int krep_gpu_format_matches_items(const void *d_pack, size_t packed_len, const krep_gpu_pack_view_t *v,
                                  const match_position_t *d_positions, uint64_t n, const krep_gpu_match_format_t *fmt /* NULL: all empty */,
                                  void *d_out, size_t out_capacity, uint64_t *d_item_out_off /* nullable */,
                                  krep_gpu_matches_out_t *out, void *stream);
/* krep_gpu_grep_batch(): what `krep [-o | -c] PATTERN` prints for every item of a batch, in item order, appended to out->bytes.
 * Mode: search_file()'s own branch (krep.c:3014-3027) — COUNT when count_lines_mode or count_matches_mode is set: prefix_i COUNT '\n'
 *   for EVERY item, zero counts and empty items included (the reference prints FILE:0); else ONLY-MATCHING when cfg->only_matching is
 *   set; else LINES.  track_positions == false outside COUNT is refused (the reference then prints its empty-match line, which no
 *   batchable search produces).
 * Taken: exactly what krep_gpu_batch_can_accelerate() takes under the same configuration, with the same reasons; every refusal comes
 *   before any device work.  -m per file stays refused with it unless krep_gpu_set_batch_max_count(1) (above: the cut, then the
 *   (start, end) order, then the formatters on the kept list), and the pack runs on cfg->device alone.
 * Per pack (the packs of krep_gpu_search_batch(): the same limit, cut between items, info->scans): packed through the staging ring,
 *   scanned once with records, ordered by start when multi-pattern, cut into item bounds, the prefixes uploaded in one copy, the pack
 *   formatted in HBM, the bytes copied straight behind out->bytes + out->len.  Under COUNT the counts are printed on the host.
 * per_item[i].count is what krep_gpu_search_batch() reports; out_offset / out_bytes locate the item's bytes relative to out->len AT
 *   ENTRY.  out->bytes is a malloc-family block (NULL with capacity 0 is fine) that the call grows.
 * Failure (a refusal, a failed allocation, copy or launch): 2 with a reason, out->len and per_item untouched, nothing partially
 *   appended across all packs.  No CPU fallback, as for krep_gpu_search_batch(). */
typedef struct krep_gpu_grep_format /* host strings; the per-item prefixes are the caller's, e.g. "FILE:" */
{
    const char *const *prefixes; /* n_items of each */
    const size_t *prefix_lens;
    krep_gpu_line_format_t line;   /* before_match, after_match, line_close (prefix must be empty)  */
    krep_gpu_match_format_t match; /* before_number, after_number, after_match (prefix must be empty) */
} krep_gpu_grep_format_t;
typedef struct krep_gpu_grep_item
{
    uint64_t count, out_offset, out_bytes;
} krep_gpu_grep_item_t;
typedef struct krep_gpu_grep_output /* malloc family; appended to */
{
    char *bytes;
    size_t len, capacity;
} krep_gpu_grep_output_t;
int krep_gpu_grep_batch(const search_params_t *params, const krep_gpu_config_t *cfg /* NULL: current */,
                        const krep_gpu_batch_item_t *items, size_t n_items, const krep_gpu_grep_format_t *fmt,
                        krep_gpu_grep_item_t *per_item /* n_items */, krep_gpu_grep_output_t *out,
                        krep_gpu_batch_info_t *info /* nullable */); /* 0, or 2 */

int krep_gpu_device_count(void);
const char *krep_gpu_last_error(void); /* "" when the last call on this thread succeeded */
void krep_gpu_clear_error(void);
const char *krep_gpu_version(void);

#ifdef __cplusplus
}
#endif
#endif /* KREP_GPU_H */
