/*
 * matchy_amd.h — C ABI of the MI355X-native `matchy match` engine (libmatchy_amd.so).
 *
 * Drop-in boundary: every `matchy_*` function declared in PART 1 keeps the name, argument meaning, ownership and
 * error convention of the reference's C API (reference = matchylabs/matchy @ 2025-12-12,
 * crates/matchy/include/matchy/matchy.h, implemented in crates/matchy/src/c_api/matchy.rs). The citation after
 * each declaration names the reference interface it replaces. PART 2 is additive (`matchy_scanner_*`): the bulk
 * entry point behind which the HIP pipeline sits; it is called exactly where the reference calls
 * Worker::process_batch (crates/matchy/src/processing/parallel.rs:411-439 -> processing/mod.rs:353-448).
 *
 * All lookups and extractions run on the GPU. There is no CPU fallback: without a usable HIP device
 * matchy_open()/matchy_extractor_create() return NULL and scanner calls return MATCHY_ERROR_IO.
 */
#ifndef MATCHY_AMD_H
#define MATCHY_AMD_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes (matchy.h:46-86) */
#define MATCHY_SUCCESS 0
#define MATCHY_ERROR_FILE_NOT_FOUND -1
#define MATCHY_ERROR_INVALID_FORMAT -2
#define MATCHY_ERROR_CORRUPT_DATA -3
#define MATCHY_ERROR_OUT_OF_MEMORY -4
#define MATCHY_ERROR_INVALID_PARAM -5
#define MATCHY_ERROR_IO -6

/* ---- extractor flags and item types (matchy.h:188-288) */
#define MATCHY_EXTRACT_DOMAINS (1 << 0)
#define MATCHY_EXTRACT_EMAILS (1 << 1)
#define MATCHY_EXTRACT_IPV4 (1 << 2)
#define MATCHY_EXTRACT_IPV6 (1 << 3)
#define MATCHY_EXTRACT_HASHES (1 << 4)
#define MATCHY_EXTRACT_BITCOIN (1 << 5)
#define MATCHY_EXTRACT_ETHEREUM (1 << 6)
#define MATCHY_EXTRACT_MONERO (1 << 7)
#define MATCHY_EXTRACT_ALL 255

#define MATCHY_ITEM_TYPE_DOMAIN 0
#define MATCHY_ITEM_TYPE_EMAIL 1
#define MATCHY_ITEM_TYPE_IPV4 2
#define MATCHY_ITEM_TYPE_IPV6 3
#define MATCHY_ITEM_TYPE_MD5 4
#define MATCHY_ITEM_TYPE_SHA1 5
#define MATCHY_ITEM_TYPE_SHA256 6
#define MATCHY_ITEM_TYPE_SHA384 7
#define MATCHY_ITEM_TYPE_SHA512 8
#define MATCHY_ITEM_TYPE_BITCOIN 9
#define MATCHY_ITEM_TYPE_ETHEREUM 10
#define MATCHY_ITEM_TYPE_MONERO 11

/* ================================================================================================
 * PART 1 — reference-compatible surface
 * ================================================================================================ */

typedef struct matchy_builder_t matchy_builder_t; /* opaque (matchy.h:293-295) */
typedef struct matchy_t matchy_t;                 /* opaque (matchy.h:396-398) */
typedef struct matchy_extractor_t matchy_extractor_t; /* opaque (matchy.h:513-515) */

/* matchy.h:361-391. auto_reload / reload_callback are accepted and ignored (watching is out of scope);
 * cache_capacity: entries of the query cache of matchy_query (LRU keyed by the query string, "not found" included; 0 disables it:
 * c_api/matchy.rs:805-808). The reference keeps one such cache per thread, this build one per handle. */
typedef struct matchy_open_options_t {
  uint32_t cache_capacity;
  bool auto_reload;
  void (*reload_callback)(const void *event, void *user_data);
  void *reload_callback_user_data;
} matchy_open_options_t;

/* matchy.h:437-454 */
typedef struct matchy_result_t {
  bool found;
  uint8_t prefix_len;
  void *_data_cache;
  const matchy_t *_db_ref;
} matchy_result_t;

/* matchy.h:520-556 */
typedef struct matchy_match_t {
  uint8_t item_type;
  const char *value;
  uintptr_t start;
  uintptr_t end;
} matchy_match_t;
typedef struct matchy_matches_t {
  const matchy_match_t *items;
  uintptr_t count;
  void *_internal;
} matchy_matches_t;

/* ---- builder (replaces c_api/matchy.rs:300-600; matchy.h:578-753) */
matchy_builder_t *matchy_builder_new(void);                                            /* matchy.h:578 */
int32_t matchy_builder_set_case_insensitive(matchy_builder_t *b, bool case_insensitive); /* matchy.h:605 */
int32_t matchy_builder_add(matchy_builder_t *b, const char *key, const char *json_data); /* matchy.h:670, c_api/matchy.rs:401-455 */
int32_t matchy_builder_set_description(matchy_builder_t *b, const char *description);   /* matchy.h:687 */
int32_t matchy_builder_save(matchy_builder_t *b, const char *filename);                 /* matchy.h:711 */
int32_t matchy_builder_build(matchy_builder_t *b, uint8_t **buffer, uintptr_t *size);   /* matchy.h:740 (buffer is malloc'ed; caller frees with free()) */
void matchy_builder_free(matchy_builder_t *b);                                          /* matchy.h:753 */

/* ---- open / close (c_api/matchy.rs:781-939, 1055-1059; matchy.h:777-938) */
void matchy_init_open_options(matchy_open_options_t *options);                                   /* matchy.h:777 */
matchy_t *matchy_open_with_options(const char *filename, const matchy_open_options_t *options);  /* matchy.h:815 (NULL options -> NULL) */
matchy_t *matchy_open(const char *filename);                                                     /* matchy.h:844 */
matchy_t *matchy_open_buffer(const uint8_t *buffer, uintptr_t size);                             /* matchy.h:863 (copies the buffer) */
void matchy_close(matchy_t *db);                                                                 /* matchy.h:938 (NULL-safe) */

/* ---- query (c_api/matchy.rs:1100-1239; matchy.h:980-1034). A single query is answered on the HOST (csrc/host_lookup.cpp: trie walk,
 * literal probe, Paraglob::find_all over the mapped sections; SURVEY §8b "single queries stay on the CPU path"): a kernel launch would cost
 * tens of microseconds where the reference answers in 0.2. Bulk work — matchy_scanner_*, matchy_extractor_extract_chunk — runs the HIP kernels. */
matchy_result_t matchy_query(const matchy_t *db, const char *query);                    /* matchy.h:980 */
void matchy_query_into(const matchy_t *db, const char *query, matchy_result_t *result); /* matchy.h:1008 */
void matchy_free_result(matchy_result_t *result);                                       /* matchy.h:1022 */
void matchy_free_string(char *string);                                                  /* matchy.h:1034 */
char *matchy_result_to_json(const matchy_result_t *result);                             /* matchy.h:1323 */

/* ---- introspection (matchy.h:1043-1190) */
const char *matchy_version(void);                                  /* matchy.h:1043 */
const char *matchy_format(const matchy_t *db);                     /* matchy.h:1059 */
bool matchy_has_ip_data(const matchy_t *db);                       /* matchy.h:1074 */
bool matchy_has_string_data(const matchy_t *db);                   /* matchy.h:1089 */
bool matchy_has_literal_data(const matchy_t *db);                  /* matchy.h:1104 */
bool matchy_has_glob_data(const matchy_t *db);                     /* matchy.h:1119 */
char *matchy_metadata(const matchy_t *db);                         /* matchy.h:1154 (JSON; free with matchy_free_string) */
char *matchy_get_pattern_string(const matchy_t *db, uint32_t id);  /* matchy.h:1173 */
uintptr_t matchy_pattern_count(const matchy_t *db);                /* matchy.h:1190 */

/* ---- extractor (c_api/matchy.rs:2270-2395; matchy.h:1380-1460). Items come back in the reference's chunk-path
 * order (IPv6, IPv4, e-mail, domain, hashes, Bitcoin, Ethereum, Monero; by position inside each class). */
matchy_extractor_t *matchy_extractor_create(uint32_t flags);                                  /* matchy.h:1380 */
int32_t matchy_extractor_extract_chunk(const matchy_extractor_t *extractor, const uint8_t *data, uintptr_t len,
                                       matchy_matches_t *matches);                             /* matchy.h:1423 */
void matchy_matches_free(matchy_matches_t *matches);                                          /* matchy.h:1434 */
void matchy_extractor_free(matchy_extractor_t *extractor);                                    /* matchy.h:1445 */
const char *matchy_item_type_name(uint8_t item_type);                                         /* matchy.h:1460 */

/* ---- statistics (matchy.h:403-432, 894, 917). cache_hits / cache_misses count the query cache of matchy_query (bulk scans do not
 * use it: their lookups run on the device). Query-type accounting follows Database::lookup (database.rs:725-804), including its
 * quirk that a miss is always counted as a string query. */
typedef struct matchy_stats_t {
  uint64_t total_queries, queries_with_match, queries_without_match, cache_hits, cache_misses, ip_queries, string_queries;
} matchy_stats_t;
void matchy_get_stats(const matchy_t *db, matchy_stats_t *stats);      /* matchy.h:894 */
void matchy_clear_cache(const matchy_t *db);                            /* matchy.h:917 */
bool matchy_has_pattern_data(const matchy_t *db);                       /* matchy.h:1137 (deprecated alias of has_string_data) */

/* ---- structured access to the data of a query result (MaxMind-style walkers, matchy.h:452-508, 1220-1290) */
#define MATCHY_ERROR_LOOKUP_PATH_INVALID (-7) /* matchy.h:163 */
#define MATCHY_ERROR_NO_DATA (-8)             /* matchy.h:168 */
#define MATCHY_ERROR_DATA_PARSE (-9)          /* matchy.h:173 */
#define MATCHY_DATA_TYPE_POINTER 1            /* matchy.h:92-157 */
#define MATCHY_DATA_TYPE_UTF8_STRING 2
#define MATCHY_DATA_TYPE_DOUBLE 3
#define MATCHY_DATA_TYPE_BYTES 4
#define MATCHY_DATA_TYPE_UINT16 5
#define MATCHY_DATA_TYPE_UINT32 6
#define MATCHY_DATA_TYPE_MAP 7
#define MATCHY_DATA_TYPE_INT32 8
#define MATCHY_DATA_TYPE_UINT64 9
#define MATCHY_DATA_TYPE_UINT128 10
#define MATCHY_DATA_TYPE_ARRAY 11
#define MATCHY_DATA_TYPE_BOOLEAN 14
#define MATCHY_DATA_TYPE_FLOAT 15
typedef union matchy_entry_data_value_u { /* matchy.h:24-36 */
  uint32_t pointer;
  const char *utf8_string;
  double double_value;
  const uint8_t *bytes;
  uint16_t uint16;
  uint32_t uint32;
  int32_t int32;
  uint64_t uint64;
  uint8_t uint128[16];
  bool boolean;
  float float_value;
} matchy_entry_data_value_u;
typedef struct matchy_entry_s { /* matchy.h:457-466 */
  const matchy_t *db;
  const void *data_ptr;
} matchy_entry_s;
typedef struct matchy_entry_data_t { /* matchy.h:471-494 */
  bool has_data;
  uint32_t type_;
  matchy_entry_data_value_u value;
  uint32_t data_size; /* string / bytes: length; map / array: element count; scalars: width */
  uint32_t offset;
} matchy_entry_data_t;
typedef struct matchy_entry_data_list_t { /* matchy.h:499-508 */
  matchy_entry_data_t entry_data;
  struct matchy_entry_data_list_t *next;
} matchy_entry_data_list_t;
int32_t matchy_result_get_entry(const matchy_result_t *result, matchy_entry_s *entry);                               /* matchy.h:1220 */
/* path = NULL-terminated array of map keys / decimal array indexes. String and byte pointers stay valid until
 * matchy_free_result (the reference leaks them instead). */
int32_t matchy_aget_value(const matchy_entry_s *entry, matchy_entry_data_t *entry_data, const char *const *path);   /* matchy.h:1245 */
/* Depth-first list: a node, then its children (map values in key order; the reference's HashMap order is unspecified). */
int32_t matchy_get_entry_data_list(const matchy_entry_s *entry, matchy_entry_data_list_t **entry_data_list);         /* matchy.h:1277 */
void matchy_free_entry_data_list(matchy_entry_data_list_t *list);                                                     /* matchy.h:1290 */

/* ---- validation (matchy.h:1357): both levels run the bounds-checked parse every open performs (header, tree size,
 * section offsets, literal / paraglob tables). *error_message (if any) is freed with matchy_free_string. */
#define MATCHY_VALIDATION_STANDARD 0 /* matchy.h:178 */
#define MATCHY_VALIDATION_STRICT 1   /* matchy.h:183 */
int32_t matchy_validate(const char *filename, int32_t level, char **error_message);
/* Schema validation of entry data is outside this build: every schema name is reported as unknown (matchy.h:86, 625). */
#define MATCHY_ERROR_UNKNOWN_SCHEMA (-8)
int32_t matchy_builder_set_schema(matchy_builder_t *builder, const char *schema_name);

/* ================================================================================================
 * PART 2 — additive bulk-scan surface (not in the reference)
 * ================================================================================================ */

typedef struct matchy_scanner_t matchy_scanner_t;

/* One match of Worker::process_bytes (processing/mod.rs:423-443): candidate span + lookup result, 16 bytes (the
 * GPU writes these records straight into pinned host memory; compact records halve the PCIe time of a scan). */
typedef struct matchy_scan_hit_t {
  uint32_t start;        /* byte offset of the matched text in the scanned buffer */
  uint32_t len_type;     /* length of the matched text in bits 0..23, MATCHY_ITEM_TYPE_* in bits 24..31 */
  uint32_t value;        /* IP results: offset of the entry data in the MMDB data section;
                            pattern results: index of the first id in pattern_ids / data_offsets */
  uint8_t kind;          /* 2 = IP result, 3 = pattern result */
  uint8_t prefix_len;    /* IP results */
  uint16_t n_ids;        /* pattern results: number of pattern ids (literal id first, then glob ids ascending) */
} matchy_scan_hit_t;
/* Limits of the record, not of the matching: a candidate text of 16 MiB or more (24-bit length) and a candidate that matches
 * more than 65535 patterns at once (16-bit id count) make the scan fail with an error instead of truncating. Glob matching
 * itself is unbounded like Paraglob::find_all (any number of results, any nesting of '*': candidates beyond what a lane of
 * the streaming pass holds are answered by a spill pass), and literal queries of case-insensitive databases are lower-cased
 * as a stream (no length limit). */
#define MATCHY_SCAN_HIT_LEN(h) ((h).len_type & 0xFFFFFFu)
#define MATCHY_SCAN_HIT_END(h) ((uint64_t)(h).start + MATCHY_SCAN_HIT_LEN(h))
#define MATCHY_SCAN_HIT_TYPE(h) ((uint8_t)((h).len_type >> 24))

/* Compact form of an IPv4 result (fetch_mode MATCHY_SCAN_FETCH_HITS | MATCHY_SCAN_FETCH_COMPACT), 8 bytes: where nearly every line
 * of a log hits an IP entry (a CIDR-heavy database) the hit records are what crosses PCIe, and half the bytes is half the time.
 * packed: offset of the entry data in the MMDB data section in bits 0..21, length of the matched text - 7 in bits 22..25 (a dotted
 * quad has 7..15 bytes), prefix length (0..32) in bits 26..31. matchy_scan_ip4_hit_expand() gives the 16-byte record back. */
typedef struct matchy_scan_ip4_hit_t {
  uint32_t start;
  uint32_t packed;
} matchy_scan_ip4_hit_t;
#define MATCHY_SCAN_IP4_DATA_BITS 22
static inline matchy_scan_hit_t matchy_scan_ip4_hit_expand(matchy_scan_ip4_hit_t c) {
  matchy_scan_hit_t h;
  h.start = c.start;
  h.len_type = (((c.packed >> MATCHY_SCAN_IP4_DATA_BITS) & 15u) + 7u) | ((uint32_t)MATCHY_ITEM_TYPE_IPV4 << 24);
  h.value = c.packed & ((1u << MATCHY_SCAN_IP4_DATA_BITS) - 1u);
  h.kind = 2;
  h.prefix_len = (uint8_t)(c.packed >> (MATCHY_SCAN_IP4_DATA_BITS + 4));
  h.n_ids = 0;
  return h;
}

typedef struct matchy_scan_result_t {
  const matchy_scan_hit_t *hits;  /* matchy_scanner_scan / fetch_mode 3: canonical order (by start, then chunk-path
                                     class order); fetch_mode 1: device order */
  size_t n_hits;
  const uint32_t *pattern_ids;
  const int64_t *data_offsets;    /* per pattern id: data-section offset or -1 */
  size_t n_ids;
  uint64_t lines;                 /* number of '\n' bytes (WorkerStats::lines_processed) */
  uint64_t candidates;            /* WorkerStats::candidates_tested */
  uint64_t bytes;
  const matchy_scan_ip4_hit_t *ip4_hits; /* MATCHY_SCAN_FETCH_COMPACT: the IPv4 results (they are NOT in `hits` then); else NULL */
  size_t n_ip4_hits;                     /* matches of the scan = n_hits + n_ip4_hits */
  void *_internal;
} matchy_scan_result_t;

/* extract_flags 0 = derive from the database like `matchy match` does (match_cmd.rs:276-303).
 * device = HIP device ordinal. Returns NULL on failure. One scanner per thread. */
matchy_scanner_t *matchy_scanner_create(const matchy_t *db, uint32_t extract_flags, int32_t device);
void matchy_scanner_free(matchy_scanner_t *scanner);
/* Scan a host buffer (copied to the device in newline-aligned pieces of < 1 GiB). len must be below 4 GiB per call
 * (hit offsets are 32 bit); feed larger inputs in batches cut at newlines, like `matchy match` does. */
int32_t matchy_scanner_scan(matchy_scanner_t *scanner, const uint8_t *data, size_t len, matchy_scan_result_t *out);
/* Scan bytes that are already resident in device memory (16-byte aligned, len < 2^31) on `hip_stream`
 * (a hipStream_t, NULL = default stream). fetch_mode: 0 = only counters are read back (n_hits is set, hits is NULL),
 * 1 = hit records in device order (like the reference, whose result order is unspecified); the arrays are BORROWED
 * from the scanner and stay valid until its next scan or matchy_scanner_free; 3 = owned copy in canonical order. */
#define MATCHY_SCAN_FETCH_COUNTS 0u
#define MATCHY_SCAN_FETCH_HITS 1u
/* 4 = the records stay in device memory: hits / pattern_ids / data_offsets are DEVICE pointers borrowed from the scanner
 * (device order, valid until its next scan), only the counters cross the bus. For consumers that aggregate or filter on the
 * GPU, and for inputs where nearly every line hits: 16 bytes per hit over PCIe otherwise bound the scan. */
#define MATCHY_SCAN_FETCH_DEVICE 4u
#define MATCHY_SCAN_FETCH_SORTED 3u
/* 1 | 8 = like 1, but the IPv4 results come as 8-byte records in ip4_hits / n_ip4_hits (same borrowing rules; device order) and
 * everything else in hits as before. Takes effect when the entry data of every IP entry lies in the first 4 MiB of the data section (22-bit offsets) —
 * otherwise, and with any other fetch mode, the flag is ignored and n_ip4_hits is 0: read both arrays. */
#define MATCHY_SCAN_FETCH_COMPACT 8u
int32_t matchy_scanner_scan_device(matchy_scanner_t *scanner, const void *device_ptr, size_t len, void *hip_stream,
                                   uint32_t fetch_mode, matchy_scan_result_t *out);
/* The two halves of matchy_scanner_scan_device: submit launches one batch on `hip_stream` and returns, wait blocks until
 * it is done and hands out its result (one batch in flight per scanner). Two scanners on two streams let one batch's
 * result transfer overlap the next batch's streaming kernel. */
int32_t matchy_scanner_submit_device(matchy_scanner_t *scanner, const void *device_ptr, size_t len, void *hip_stream,
                                     uint32_t fetch_mode);
int32_t matchy_scanner_wait(matchy_scanner_t *scanner, matchy_scan_result_t *out);
void matchy_scan_result_free(matchy_scan_result_t *result);
/* true for a result of fetch_mode MATCHY_SCAN_FETCH_DEVICE: hits / pattern_ids / data_offsets are DEVICE pointers and must not be
 * dereferenced on the host (matchy_scan_hit_to_json returns NULL for such a result). */
bool matchy_scan_result_on_device(const matchy_scan_result_t *result);
/* The NDJSON record `matchy match` prints for hit i (match_processor/parallel.rs:297-369). `text` points at the
 * scanned bytes on the host. Returned string: matchy_free_string(). */
char *matchy_scan_hit_to_json(const matchy_scanner_t *scanner, const matchy_scan_result_t *result, size_t i,
                              const uint8_t *text, const char *source);
/* Every match of a result as NDJSON — the line matchy_scan_hit_to_json returns for each hit, in the order of the arrays (hits, then
 * ip4_hits), '\n' behind every line — in one call: *out is a malloc'ed buffer of *out_len bytes (NUL behind them), released with
 * matchy_free_string. The scanner caches the rendered data payloads by data offset (not thread-safe per scanner, like its scans). */
int32_t matchy_scan_result_to_ndjson(matchy_scanner_t *scanner, const matchy_scan_result_t *result, const uint8_t *text,
                                     const char *source, char **out, size_t *out_len);
/* ---- Line context (opt-in, off by default: with it off a scan launches and allocates nothing more and returns what it always did).
 * For every hit of a scan: the 0-based index of its line in the scanned buffer (= number of '\n' bytes in front of the hit), where
 * that line starts, and where it ends (the position of its '\n', or the length of the buffer for an unterminated last line; a '\r'
 * in front of the '\n' belongs to the line). Per scan: the number of distinct lines with at least one hit (WorkerStats::
 * lines_with_matches). All of it is computed on the GPU from the batch that is resident there. */
typedef struct matchy_scan_line_t { uint32_t line, line_start, line_end, reserved; } matchy_scan_line_t;
/* Applies to the scanner's next scan through every entry (matchy_scanner_scan, _scan_device, _submit_device: read at submit). A result
 * of a scan with line context owns a small block even where its arrays are borrowed: release it with matchy_scan_result_free. */
void matchy_scanner_set_line_context(matchy_scanner_t *scanner, bool enabled);
bool matchy_scanner_line_context(const matchy_scanner_t *scanner);
/* lines[i] belongs to result->hits[i]; ip4_lines[i] to result->ip4_hits[i] (NULL without compact records). Same ownership and
 * lifetime as the hit arrays of that result (borrowed / owned / device pointers for MATCHY_SCAN_FETCH_DEVICE; NULL for
 * MATCHY_SCAN_FETCH_COUNTS, which still delivers lines_with_matches). MATCHY_ERROR_INVALID_PARAM if the result was produced with
 * line context off. Any out pointer may be NULL. */
int32_t matchy_scan_result_lines(const matchy_scan_result_t *result, const matchy_scan_line_t **lines,
                                 const matchy_scan_line_t **ip4_lines, uint64_t *lines_with_matches);
/* matchy_scan_result_to_ndjson with "line_number" (line_base + line + 1: 1-based when line_base is the number of lines in front of
 * the scanned buffer) and, if with_input_line, "input_line" in every record: the bytes of the line, converted like
 * String::from_utf8_lossy (one U+FFFD per maximal ill-formed subsequence). Keys stay sorted: cidr, data, input_line, line_number,
 * match_type, ... . The result must come from a scan with line context and be host-resident. */
int32_t matchy_scan_result_to_ndjson_lines(matchy_scanner_t *scanner, const matchy_scan_result_t *result, const uint8_t *text,
                                           const char *source, uint64_t line_base, bool with_input_line, char **out, size_t *out_len);
/* With matchy_scanner_set_profile: milliseconds of the streaming '\n' count, the prefix sum, and resolve + distinct set of the last scan. */
void matchy_scanner_get_line_timing(const matchy_scanner_t *scanner, float out_ms[3]);
/* ---- Hit lines (opt-in, off by default: a scanner that never enabled it allocates, launches and copies nothing more, and every other
 * output stays byte for byte what it is). A caller that renders records needs the bytes of the lines that hit, not the batch: a pass
 * behind line context packs the DISTINCT lines with at least one hit into one contiguous block on the GPU, in ascending line order,
 * each ended by one '\n', and only that block and small index arrays cross the bus. With n_lines == lines_with_matches lines k = 0 ..
 * n_lines - 1:
 *   text[line_off[k] .. line_off[k+1] - 1) are the bytes batch[line_start .. line_end) of the line (a '\r' in front of the '\n' belongs
 *   to it, as in matchy_scan_line_t); text[line_off[k+1] - 1] == '\n' always, also for an unterminated last line;
 *   line_off[n_lines] == text_len, and text_len <= len + 1 (the lines are disjoint pieces of the batch and only an unterminated last
 *   line gains a byte), so the offsets are 32-bit; line_no[k] is the line's index in the batch, strictly ascending;
 *   line_of_hit[i] / line_of_ip4_hit[i] give k for hits[i] / ip4_hits[i], in the order of those arrays.
 * The text of hit i lies at text + line_off[k] + (hits[i].start - lines[i].line_start), with lines from matchy_scan_result_lines: a
 * match never spans a '\n'. The block depends on the batch and the set of hits alone, not on the order of the device's records. */
typedef struct matchy_scan_hit_lines_t {
  const uint8_t *text;
  uint64_t text_len;
  uint32_t n_lines;
  const uint32_t *line_off, *line_no, *line_of_hit, *line_of_ip4_hit;
} matchy_scan_hit_lines_t;
/* Applies to the scanner's next scan through every entry (read at submit, like line context, which it turns on for that scan: the
 * result also answers matchy_scan_result_lines). */
void matchy_scanner_set_hit_lines(matchy_scanner_t *scanner, bool enabled);
bool matchy_scanner_hit_lines(const matchy_scanner_t *scanner);
/* Ownership, lifetime and residency follow the hit arrays of the result, as for matchy_scan_result_lines: borrowed from the scanner
 * until its next scan, owned by the result for MATCHY_SCAN_FETCH_SORTED and matchy_scanner_scan, DEVICE pointers (text included; nothing
 * of the block is copied) for MATCHY_SCAN_FETCH_DEVICE. For MATCHY_SCAN_FETCH_COUNTS the gather does not run: the pointers are NULL,
 * text_len is 0 and n_lines = lines_with_matches. MATCHY_ERROR_INVALID_PARAM for a result produced with the setting off.
 * For a host-resident result that carries hit lines, matchy_scan_hit_to_json and the matchy_scan_result_to_ndjson* calls take the
 * matched text and "input_line" from the block and ignore `text`, which may be NULL; their output is what the whole batch gives. */
int32_t matchy_scan_result_hit_lines(const matchy_scan_result_t *result, matchy_scan_hit_lines_t *out);
/* With matchy_scanner_set_profile: milliseconds of the index steps (mark, rank, lengths, offsets), of the copy kernel, and of the
 * block's device-to-host copy (0 where nothing is copied) of the last scan. */
void matchy_scanner_get_hit_lines_timing(const matchy_scanner_t *scanner, float out_ms[3]);
/* ---- Rendered records: the records of a scan leave the device as NDJSON text.
 * The text is the one matchy_scan_result_to_ndjson / _lines / _segments give for the same result, byte for byte: one line per record, in
 * the order of `hits`, then `ip4_hits`. The payload JSON of the database's entries is made by the host once per data offset and kept in
 * device memory across scans; everything else of a record is written by the GPU (csrc/render.hip). */
#define MATCHY_RENDER_LINE_NUMBERS 1u   /* "line_number": needs line context (matchy_scanner_set_line_context) */
#define MATCHY_RENDER_INPUT_LINE   2u   /* "input_line" as well (implies LINE_NUMBERS) */
typedef struct matchy_render_params_t {
  uint32_t flags;
  const char *source;            /* one source (NULL = "-"), or */
  const char *const *sources;    /* one per segment of the scan it arms (then `source` is ignored) */
  size_t n_sources;
  uint64_t line_base;            /* lines in front of the buffer; or, with sources, */
  const uint64_t *line_bases;    /* one per segment (NULL = zeros) */
} matchy_render_params_t;
/* Arms the scanner's NEXT scan through matchy_scanner_scan, _scan_device, _submit_device, _scan_gz or _scan_gz_files (the parameters are copied at the
 * call; NULL disarms), and that scan consumes them whether it succeeds or not. A scan armed with parameters that do not fit it — line flags without
 * line context, `sources` for a scan without segments, n_sources other than the segment count — fails with MATCHY_ERROR_INVALID_PARAM
 * and a message; the scanner stays usable. matchy_scanner_scan renders piece by piece and hands out the blocks end to end. */
int32_t matchy_scanner_set_render(matchy_scanner_t *scanner, const matchy_render_params_t *params);
#define MATCHY_RENDER_OK 0
#define MATCHY_RENDER_TOO_LARGE 1   /* more text than MATCHY_AMD_RENDER_MAX_BYTES (default 1 GiB), more distinct payloads in one batch than
                                       MATCHY_AMD_RENDER_PAYLOADS (default 2^20), or a "data" array above 16 MiB: nothing is handed out */
/* The block of a result whose scan was armed. Ownership and residency follow the hit arrays of the result: borrowed until the scanner's
 * next scan, owned by the result for MATCHY_SCAN_FETCH_SORTED and matchy_scanner_scan, a device pointer with nothing copied for MATCHY_SCAN_FETCH_DEVICE; a
 * MATCHY_SCAN_FETCH_COUNTS fetch renders nothing (text NULL, len 0). MATCHY_ERROR_INVALID_PARAM for a result whose scan was not armed.
 * Any out pointer may be NULL. */
int32_t matchy_scan_result_ndjson(const matchy_scan_result_t *result, const char **text, uint64_t *len, int32_t *status);
/* With matchy_scanner_set_profile: milliseconds of measure + offsets, of the write step, and of the block's device-to-host copy (0 where
 * nothing is copied) of the last scan that rendered. */
void matchy_scanner_get_render_timing(const matchy_scanner_t *scanner, float out_ms[3]);
/* Of the last scan that rendered: repeats of the pass (0 in the steady state), payload-table misses over all its rounds, payloads the
 * host rendered and uploaded, bytes of the block copied to the host, growths of the payload table's slot array and of its device pool
 * (they start at MATCHY_AMD_RENDER_PAYLOADS_SLOTS = 64 slots and MATCHY_AMD_RENDER_PAYLOADS_POOL_BYTES = 64 KiB; the variables are for tests). */
void matchy_scanner_get_render_counters(const matchy_scanner_t *scanner, uint64_t out[6]);
/* ---- Segmented scans: many small inputs as one batch.
 * The caller describes a buffer as a sequence of segments (the files of a pack): the scan runs once, as for any buffer, and a pass
 * behind it attributes every hit record to its segment on the GPU and counts per segment. '\n' is a boundary for every extractor, so
 * scanning "A\nB\n" finds exactly the matches of "A\n" and of "B\n". */
typedef struct matchy_scan_segment_t {
  uint32_t start, len;          /* as given (len = next start - start; the last one ends at the buffer's end) */
  uint32_t hits;                /* matches whose start lies in the segment (records of `hits` and `ip4_hits` together) */
  uint32_t line_base;           /* '\n' bytes in front of `start`            — line context only, else 0 */
  uint32_t lines;               /* '\n' bytes inside the segment              — line context only, else 0 */
  uint32_t lines_with_matches;  /* distinct lines of the segment with a hit   — line context only, else 0 */
  uint32_t reserved[2];
} matchy_scan_segment_t;
/* Copies the table; it applies to the scanner's NEXT scan only, through every entry (matchy_scanner_scan, _scan_device,
 * _submit_device: read at submit), and that scan consumes it whether it succeeds or not. n == 0 or starts == NULL clears a pending
 * table. Required: starts[0] == 0, non-decreasing (equal neighbours are empty segments), every start <= the scan's len, and every
 * non-empty segment in front of the last ends in '\n'. A table that breaks a rule fails that scan with MATCHY_ERROR_INVALID_PARAM
 * and a message (the newline rule is checked on the device, one byte per segment; the message names the first offending segment);
 * the scanner stays usable. Extraction-only scans and single queries ignore segments. */
int32_t matchy_scanner_set_segments(matchy_scanner_t *scanner, const uint32_t *starts, size_t n);
/* segment_of_hit[i] belongs to result->hits[i], segment_of_ip4_hit[i] to result->ip4_hits[i]: the LAST segment whose start is <= the
 * hit's start (an empty segment never owns a hit). Ownership, lifetime and residency follow the hit arrays of the result, as for
 * matchy_scan_result_lines (NULL for MATCHY_SCAN_FETCH_COUNTS). `segments` is host memory owned by the result, n_segments entries,
 * filled for every fetch mode. The line of a hit inside its segment is lines[i].line - segments[s].line_base. MATCHY_ERROR_INVALID_PARAM
 * for a result of a scan without segments. Any out pointer may be NULL. */
int32_t matchy_scan_result_segments(const matchy_scan_result_t *result, const uint32_t **segment_of_hit, const uint32_t **segment_of_ip4_hit,
                                    const matchy_scan_segment_t **segments, size_t *n_segments);
/* matchy_scan_result_to_ndjson with sources[segment] as the source of each record. line_bases != NULL: the result must carry line
 * context, and the records are those of matchy_scan_result_to_ndjson_lines with
 * "line_number" = line_bases[s] + (line - segments[s].line_base) + 1. */
int32_t matchy_scan_result_to_ndjson_segments(matchy_scanner_t *scanner, const matchy_scan_result_t *result, const uint8_t *text,
                                              const char *const *sources, const uint64_t *line_bases, bool with_input_line,
                                              char **out, size_t *out_len);
/* With matchy_scanner_set_profile: milliseconds of the segment pass, the record passes and the lines-with-matches pass of the last scan. */
void matchy_scanner_get_segment_timing(const matchy_scanner_t *scanner, float out_ms[3]);
/* ---- gz scans: many compressed files, one scan (opt-in: with these calls never made a scanner allocates, launches and copies nothing
 * more, and every output stays as it is).
 * The caller hands over one host buffer that holds whole gzip files (RFC 1952, one member each) and a table of them. The compressed
 * bytes cross the bus, one wave per file inflates it on the GPU into its segment of one batch in device memory, CRC-32 and ISIZE are
 * verified there, and the scan runs over that batch as a segmented scan: segment i is member i. DEFLATE is sequential within a
 * stream: the parallelism is across the files, and a single large file gains nothing without pieces
 * (matchy_scanner_set_gz_pieces, below) — and with them still nothing where its stream has no dynamic block at which a piece can start.
 * Layout of the batch: the members' texts end to end in table order, one '\n' — the separator, which is not the input's — behind every
 * non-empty member, whether or not its text ends in one: start[0] = 0, start[i + 1] = start[i] + out_len[i] + 1 for a non-empty
 * member and start[i] for an empty one. Line numbers inside a member do not change: the extra empty line is its last.
 * out_len: 0 = take the capacity from ISIZE, the member's last four bytes (what `matchy match --gz-on-gpu` does); any other value is
 * the inflated length the caller vouches for. A member that inflates to more or fewer bytes fails.
 * A member that fails does not fail the call: it gets a status, its whole region of the batch is overwritten with '\n' so that it can
 * contribute no hit, and it keeps its index. One status per member; the FIRST error in stream order decides, and behind a stream that
 * ended the trailer checks run in the order TRUNCATED, SIZE_MISMATCH, CRC_MISMATCH, TRAILING_DATA. */
#define MATCHY_GZ_OK 0
#define MATCHY_GZ_BAD_HEADER 1     /* host: the gzip header does not parse (magic, CM != 8, reserved FLG bit, a field past the end) */
#define MATCHY_GZ_TRUNCATED 2      /* the input ends before the stream or its trailer does */
#define MATCHY_GZ_BAD_BLOCK 3      /* block type 3, LEN / NLEN mismatch */
#define MATCHY_GZ_BAD_CODES 4      /* bad code lengths or tables (what zlib's inflate_table refuses, and the rules of the code-length code) */
#define MATCHY_GZ_BAD_SYMBOL 5     /* length symbol 286 / 287, distance symbol 30 / 31, bits that are no code of an incomplete code */
#define MATCHY_GZ_BAD_DISTANCE 6   /* back-reference beyond the bytes produced */
#define MATCHY_GZ_OVERFLOW 7       /* more output than out_len */
#define MATCHY_GZ_SIZE_MISMATCH 8  /* fewer bytes than out_len, or the trailer's ISIZE differs */
#define MATCHY_GZ_CRC_MISMATCH 9   /* the trailer's CRC-32 differs */
#define MATCHY_GZ_TRAILING_DATA 10 /* bytes behind the trailer: a second member or garbage (gzread would go on; the caller falls back) */
typedef struct matchy_gz_member_t { uint64_t offset; uint32_t len; uint32_t out_len; } matchy_gz_member_t;
/* fetch_mode as matchy_scanner_scan_device (every mode; line context and the tally apply as for any scan). The result answers
 * matchy_scan_result_segments (and _lines) like any segmented scan, and matchy_scan_result_gz. Its `lines` counts the '\n' bytes of the
 * OK members' own text (separators and overwritten regions are not counted), its `bytes` is the sum of the OK members' inflated
 * lengths; offsets of hits are offsets into the batch. want_text: the inflated batch is copied to pinned host memory once, behind the
 * scan, for matchy_scan_hit_to_json and the NDJSON calls; without it only counters, records and tables cross the bus.
 * MATCHY_ERROR_INVALID_PARAM with a message, and a scanner that stays usable: NULL handles, n == 0, a member outside packed[0, packed_len),
 * a batch that reaches 2^31 bytes. */
int32_t matchy_scanner_scan_gz(matchy_scanner_t *scanner, const uint8_t *packed, size_t packed_len, const matchy_gz_member_t *members,
                               size_t n, uint32_t fetch_mode, bool want_text, matchy_scan_result_t *out);
/* status: n_members values MATCHY_GZ_*, owned by the result. text / text_len: the inflated batch — NULL / its length without want_text;
 * borrowed from the scanner until its next scan, or owned by the result for MATCHY_SCAN_FETCH_SORTED (like the hit arrays of that mode).
 * MATCHY_ERROR_INVALID_PARAM for a result of another kind of scan. Any out pointer may be NULL. */
int32_t matchy_scan_result_gz(const matchy_scan_result_t *result, const int32_t **status, size_t *n_members, const uint8_t **text,
                              size_t *text_len);
/* With matchy_scanner_set_profile: milliseconds of the inflate kernel (the CRC is computed inside it), 0, and the seal kernel (of a scan
 * of files: the verdict and seal kernels) of the last gz scan. */
void matchy_scanner_get_gz_timing(const matchy_scanner_t *scanner, float out_ms[3]);
/* ---- gz scans of multi-member files (opt-in, beside matchy_scanner_scan_gz, which stays as it is): a gzip file may hold many members
 * (RFC 1952: `cat a.gz b.gz`, `pigz -i`, appended chunks, BGZF), each an independent DEFLATE stream, so a file of k members is inflated
 * by k waves. The table names whole FILES; the library finds the members of each on the host (a BGZF header names its member's length;
 * otherwise the next 1f 8b 08 with no reserved FLG bit, XFL 0 / 2 / 4 and a header that parses, at least 10 bytes behind the body's
 * start; FNAME and FCOMMENT of a later member count up to 256 bytes each, so the search is linear in the file's length whatever it
 * holds). A cut is a guess the device verifies: a member must end exactly 8 bytes before its piece's end, and its CRC-32 and ISIZE must
 * match — a false cut cannot yield pieces that are all OK. A file is OK when all its members are; otherwise it takes the status of its
 * first member in stream order that is not, its whole region is overwritten with '\n', and the caller falls back (gzread) for it.
 * Layout of the batch: segment i is FILE i. The members of a file lie end to end with nothing between them (a line may span two
 * members); one '\n' — the separator — follows every file whose inflated length is not 0. Every capacity is the member's own ISIZE.
 * `lines` and `bytes` count the OK files' own text. Fetch modes, line context, hit lines, rendered records, the tally, the refusal of
 * whole-line queries and the errors are those of matchy_scanner_scan_gz; a file of 4 GiB or more is refused as well. */
typedef struct matchy_gz_file_t { uint64_t offset; uint64_t len; } matchy_gz_file_t;
int32_t matchy_scanner_scan_gz_files(matchy_scanner_t *scanner, const uint8_t *packed, size_t packed_len, const matchy_gz_file_t *files,
                                     size_t n_files, uint32_t fetch_mode, bool want_text, matchy_scan_result_t *result);
/* file_status: n_files values MATCHY_GZ_*; first_member: n_files + 1 values, the members of file f are [first_member[f],
 * first_member[f + 1]) of what matchy_scan_result_gz hands out (per-member statuses, and the text as for any gz scan). Owned by the
 * result. MATCHY_ERROR_INVALID_PARAM for a result of another kind of scan. Any out pointer may be NULL. */
int32_t matchy_scan_result_gz_files(const matchy_scan_result_t *result, const int32_t **file_status, size_t *n_files,
                                    const uint32_t **first_member);
/* ---- gz windows (opt-in, beside the calls above, which stay as they are): a multi-member file that is LARGER than one batch is scanned
 * as a chain of windows. A window is a run of consecutive whole members of ONE file; the caller cuts the file (it only needs member
 * boundaries: BGZF names them, csrc/gz_plan.h gz_next_window walks them) so that the window's text plus the carry fits a batch, and
 * scans the windows one after another. packed[0, packed_len) holds the window's whole members; the library splits it into members
 * itself, as matchy_scanner_scan_gz_files does for a file, and the device verifies every cut. Layout of the batch:
 *   [carry][member 0 text] ... [member m-1 text][one '\n' separator, only with MATCHY_WINDOW_LAST and carry + text > 0]
 * Behind the inflate, verdict and seal kernels, k_gz_window_tail finds the window's last '\n', copies the partial line behind it — the
 * carry, at most carry_cap bytes — out and overwrites it with '\n'; the caller hands that carry to the NEXT window, so every line lies
 * whole in exactly one batch. The window is ONE segment that starts at 0. `bytes` is carry_len + inflated length - the new carry's length
 * and `lines` the '\n' bytes of that range, so over the windows of a file they sum to the file's inflated length and line count.
 * Outcomes:  members not all OK (matchy_scan_result_gz_files: one file): the whole batch, carry included, is '\n': no hit, bytes 0, an
 *            empty carry; the caller falls back (gzread) from the bytes the windows in front consumed.
 *            MATCHY_WINDOW_NO_LINE_END: more than carry_cap bytes lie behind the window's last '\n' (or the window is longer than
 *            carry_cap and has none): the same — all '\n', no hit, bytes 0, empty carry.
 *            MATCHY_WINDOW_LAST: nothing is cut; the last partial line is scanned, the carry is empty.
 * The result also answers matchy_scan_result_gz_files (one file), matchy_scan_result_gz (member statuses; the text, carry included) and
 * matchy_scan_result_segments (one segment). Windows of one file are serial: each needs the carry of the one in front. Fetch modes, line
 * context, hit lines, rendered records, the tally and the refusal of whole-line queries are those of matchy_scanner_scan_gz.
 * MATCHY_ERROR_INVALID_PARAM with a message, and a scanner that stays usable: NULL handles, packed_len == 0, carry_len > carry_cap,
 * carry == NULL with carry_len > 0, a batch that reaches 2^31 bytes (the carry counted), unknown flag bits. */
#define MATCHY_WINDOW_LAST 1u          /* flags: the file ends with this window */
#define MATCHY_WINDOW_OK 0
#define MATCHY_WINDOW_NO_LINE_END 1    /* more than carry_cap bytes behind the window's last '\n' (or none at all in a window longer than carry_cap) */
typedef struct matchy_gz_window_t { const uint8_t *carry; uint32_t carry_len, carry_cap, flags; } matchy_gz_window_t;
int32_t matchy_scanner_scan_gz_window(matchy_scanner_t *scanner, const uint8_t *packed, size_t packed_len, const matchy_gz_window_t *window,
                                      uint32_t fetch_mode, bool want_text, matchy_scan_result_t *result);
/* window_status: MATCHY_WINDOW_*; carry / carry_len: the bytes behind the window's last '\n', owned by the result (valid until it is
 * freed). MATCHY_ERROR_INVALID_PARAM for a result of another kind of scan. Any out pointer may be NULL. */
int32_t matchy_scan_result_gz_window(const matchy_scan_result_t *result, int32_t *window_status, const uint8_t **carry, size_t *carry_len);
/* matchy_scanner_get_gz_timing behind a window scan (out_ms[2] then includes k_gz_window_tail), and that kernel's own milliseconds as
 * out_ms[3]. */
void matchy_scanner_get_gz_window_timing(const matchy_scanner_t *scanner, float out_ms[4]);
/* ---- pieces of one stream (opt-in, beside the calls above: with piece_bytes 0, the default, every kernel launch, status and output
 * byte is what it is without this call). A large member is cut into pieces of piece_bytes compressed bytes. Every piece but the first
 * looks for the first bit position inside it where a dynamic DEFLATE block header parses, and all pieces are decoded at once from there
 * into 16-bit symbols, a back-reference into the unknown 32 KiB in front becoming a marker; a piece stops at the block end that is the
 * start of a later piece. The pieces reached from piece 0 this way form a chain that is the sequential parse of the stream; markers are
 * then resolved down the chain, and CRC-32 and ISIZE are verified as ever. A member whose chain does not reach the stream's end, or
 * that fails any test on the way, is inflated afterwards in the same scan by the one-wave path, whose status it gets: there is no new
 * status value, and output, statuses and their precedence are those of the scan with pieces off.
 * piece_bytes: 0 = off; a power of two from 512 to 1 MiB = on for every member of at least 2 * piece_bytes compressed bytes; anything
 * else is MATCHY_ERROR_INVALID_PARAM and the setting (and the scanner) stays as it was. It applies to matchy_scanner_scan_gz,
 * matchy_scanner_scan_gz_files and matchy_scanner_scan_gz_window, whose members go through the same inflate stage.
 * Limits. Stored and fixed blocks have no findable start: the piece in front decodes through them, so a stream of such blocks alone
 * (gzip -1 on some builds, zlib Z_FIXED) is decoded by piece 0 at one wave's pace and costs the find on top. A member that is handed
 * over costs what it costs with pieces off, plus the passes that ran. The symbol scratch is 2 bytes per inflated byte of the split
 * members (at most 4 GiB, which a batch below 2^31 bytes never reaches). What a batch cannot hold stays outside
 * this call: a member larger than a batch. A single-stream file larger than a batch is scanned as a chain of stream windows
 * (matchy_scanner_scan_gz_stream, below), which need this setting on. */
typedef struct matchy_gz_piece_t {
    uint64_t start_bit, end_bit;  /* in the member's DEFLATE body; end_bit: where its decoder stopped. 0 without MATCHY_PIECE_HAS_START */
    uint32_t member;              /* index into the statuses of matchy_scan_result_gz */
    uint32_t produced, out_pos;   /* bytes it decoded; where they begin in the member's text (0 unless live) */
    uint32_t flags;               /* MATCHY_PIECE_* */
} matchy_gz_piece_t;
#define MATCHY_PIECE_HAS_START 1u    /* a block start was found in it (piece 0 of a member: always) */
#define MATCHY_PIECE_LIVE 2u         /* on the chain from piece 0 */
#define MATCHY_PIECE_HANDED_OVER 4u  /* its member was inflated by the one-wave path after all */
int32_t matchy_scanner_set_gz_pieces(matchy_scanner_t *scanner, uint32_t piece_bytes);
uint32_t matchy_scanner_get_gz_pieces(const matchy_scanner_t *scanner);
/* The piece table of a gz scan, owned by the result: n pieces, laid out member by member; first_piece: n_members + 1 values, the pieces
 * of member i are [first_piece[i], first_piece[i + 1]) — none for a member that was not split. With pieces off n is 0 and first_piece
 * NULL. MATCHY_ERROR_INVALID_PARAM for a result of another kind of scan. Any out pointer may be NULL. */
int32_t matchy_scan_result_gz_pieces(const matchy_scan_result_t *result, const matchy_gz_piece_t **pieces, size_t *n, const uint32_t **first_piece);
/* With matchy_scanner_set_profile: milliseconds of the find, count, chain and symbols kernels, of windows + resolve + verdict, and of the
 * handover inflate of the last gz scan (all part of out_ms[0] of matchy_scanner_get_gz_timing); zeros where no member was split. */
void matchy_scanner_get_gz_pieces_timing(const matchy_scanner_t *scanner, float out_ms[6]);
/* ---- stream windows (opt-in, beside the calls above, which stay as they are; matchy_scanner_set_gz_pieces must be on): ONE DEFLATE
 * stream that is larger than a batch — what `gzip access.log` writes — is scanned as a chain of windows. A window is a run of the
 * stream's compressed bytes whose first block starts at bit `bit` of its first byte; what the windows in front produced is the STATE:
 * the text's length, its CRC-32 and its last 32 KiB. The device cuts the window into pieces as for a split member, piece 0 starting at
 * that bit with the state's history in reach, follows the chain of pieces as far as the window's bytes and text_cap carry it, resolves
 * markers (piece 0's from the history), folds the CRC into the state's and reports where it stopped: consumed_bits, counted from bit 0
 * of packed[0], the gzip header of the first window included. The NEXT window starts at byte consumed_bits / 8 of this one with
 * bit = consumed_bits % 8 and the state handed out (csrc/gz_stream.h decides how many bytes it gets). The stream's end counts only in a
 * window that carries MATCHY_STREAM_FILE_END: there the trailer is verified — exactly 8 bytes behind the last block, ISIZE equal to the
 * whole text's length modulo 2^32, the CRC-32 of the whole text — with the precedence of every gz scan. Layout of the batch, one segment:
 *   [carry][window text][one '\n' separator, only where the stream ended here and carry + text > 0]
 * and, because the text's length is known on the device only, '\n' up to carry_len + text_cap + 1 bytes, which is what is scanned; `bytes`
 * and `lines` follow the accounting of matchy_scanner_scan_gz_window, so over the windows of a file they sum to its inflated length and
 * line count. The carry is the partial line behind the window's last '\n', as there.
 * Outcomes:  MATCHY_STREAM_OK           text scanned; consumed_bits, text_len, ended, the new state and the new carry are handed out
 *            MATCHY_STREAM_NO_PROGRESS  no piece was taken: the window holds no whole block that ends on a found block start (a stream of
 *                                       stored or fixed blocks has none), or one block is larger than text_cap
 *            MATCHY_STREAM_NO_LINE_END  as MATCHY_WINDOW_NO_LINE_END
 *            MATCHY_STREAM_FAILED       gz_status names it: a header that does not parse (first window, on the host), a stream error in
 *                                       the window's first block, a distance in front of the stream's first byte, or the trailer
 *            In all but the first the whole batch is '\n': no hit, bytes 0, an empty carry, no state; the caller falls back (gzread)
 *            from the text the windows in front gave. Windows in front stay reported: a failing trailer is seen in the last window.
 * The result also answers matchy_scan_result_gz (one member: gz_status; the text, carry included), matchy_scan_result_gz_pieces (the
 * window's pieces; bits relative to the window's first DEFLATE byte) and matchy_scan_result_segments. Fetch modes, line context, hit
 * lines, rendered records, the tally and the refusal of whole-line queries are those of matchy_scanner_scan_gz_window. The symbol scratch
 * is 2 * text_cap bytes. MATCHY_ERROR_INVALID_PARAM with a message, and a scanner that stays usable: NULL handles, packed_len == 0 or
 * 4 GiB and more, pieces off, carry_len > carry_cap, carry == NULL with carry_len > 0, text_cap == 0, carry_len + text_cap reaching 2^31,
 * no state without MATCHY_STREAM_FIRST, state->bit > 7, history_len > 32768 or > text_bytes, unknown flag bits. */
typedef struct matchy_gz_stream_state_t { uint64_t text_bytes; uint32_t crc, bit, history_len; uint8_t history[32768]; } matchy_gz_stream_state_t;
typedef struct matchy_gz_stream_window_t {
    const matchy_gz_stream_state_t *state;   /* NULL with MATCHY_STREAM_FIRST (it is not read then) */
    const uint8_t *carry; uint32_t carry_len, carry_cap, text_cap, flags;
} matchy_gz_stream_window_t;
#define MATCHY_STREAM_FIRST 1u      /* packed begins with the gzip header (parsed on the host: MATCHY_GZ_BAD_HEADER as elsewhere) */
#define MATCHY_STREAM_FILE_END 2u   /* packed reaches the file's last byte */
#define MATCHY_STREAM_OK 0
#define MATCHY_STREAM_NO_LINE_END 1
#define MATCHY_STREAM_NO_PROGRESS 2
#define MATCHY_STREAM_FAILED 3
int32_t matchy_scanner_scan_gz_stream(matchy_scanner_t *scanner, const uint8_t *packed, size_t packed_len, const matchy_gz_stream_window_t *window,
                                      uint32_t fetch_mode, bool want_text, matchy_scan_result_t *result);
/* status: MATCHY_STREAM_*; gz_status: MATCHY_GZ_*; text_len: the window's inflated bytes; state_out, carry: owned by the result (valid
 * until it is freed), meaningful for MATCHY_STREAM_OK (state_out is NULL otherwise). MATCHY_ERROR_INVALID_PARAM for a result of another
 * kind of scan. Any out pointer may be NULL. */
int32_t matchy_scan_result_gz_stream(const matchy_scan_result_t *result, int32_t *status, int32_t *gz_status, uint64_t *consumed_bits, uint32_t *text_len,
                                     bool *ended, const matchy_gz_stream_state_t **state_out, const uint8_t **carry, size_t *carry_len);
/* With matchy_scanner_set_profile: milliseconds of the passes of the last stream window: find, count, chain, symbols, windows, resolve,
 * verdict, line tail; zeros where none ran. */
#define MATCHY_STREAM_PASSES 8
void matchy_scanner_get_gz_stream_timing(const matchy_scanner_t *scanner, float out_ms[MATCHY_STREAM_PASSES]);
/* Per-kernel HIP-event timing of the last scan (recorded on the scan's stream):
 * out[0..4] = k_anchor, k_validate_dom + k_validate, k_rare, k_lookup (incl. writing the hit records), total (milliseconds).
 * matchy_scanner_scan_device runs the kernels behind k_anchor on three streams: then out[1] is that whole tail and out[2] = out[3] = 0. */
void matchy_scanner_set_profile(matchy_scanner_t *scanner, bool enabled);
/* matchy_scanner_scan_device cuts a large batch into slices and runs the kernels behind the streaming pass of one slice beside
 * the streaming pass of the next (results do not depend on it: N4 of the design notes, positions stay absolute). 0 = default for
 * the batch size, 1 = never cut, n = n equal slices (at most 8). matchy_scanner_last_slices: what the last scan used. */
void matchy_scanner_set_slices(matchy_scanner_t *scanner, int32_t slices);
int32_t matchy_scanner_last_slices(const matchy_scanner_t *scanner);
void matchy_scanner_get_timing(const matchy_scanner_t *scanner, float out_ms[5]);
/* Last error message of the calling thread ("" if none). */
/* `matchy query DB QUERY` (bin/commands/query_cmd.rs:8-69) as one call: compact JSON array — one object per matching
 * pattern that carries data (literal first, then globs by id), or the IP entry's data plus "cidr" and "prefix_len", or
 * [] — and *found = the command's exit-status rule. Free with matchy_free_string. NULL on error. */
char *matchy_amd_query_json(const matchy_t *db, const char *query, int32_t *found);
/* matchy_extractor_create with ExtractorBuilder::min_domain_labels (matchy-extractor/src/lib.rs:101-104;
 * `matchy extract --min-labels`); 0 = the default of 2. */
matchy_extractor_t *matchy_amd_extractor_create(uint32_t flags, uint32_t min_domain_labels);
/* Distinct candidates (`matchy extract --unique`). While enabled, matchy_extractor_extract_chunk returns only the candidates that are
 * the first occurrence of their text — the raw bytes data[start, end), case-sensitive, whatever the item type; for IP addresses the
 * text in the log, not the canonical value — since the handle was created or reset; order and fields are as without it. The set of
 * texts lives in device memory, owned by the handle, across calls; among the occurrences of a text in one call the one with the
 * least (start, extractor order) stays. Disabled (the default) nothing is allocated, launched or copied for it; switching it off
 * keeps the set, _reset_unique empties it (and keeps its allocations), matchy_extractor_free releases it. _unique_count: distinct
 * texts seen since creation or reset. Like extract_chunk these serialise on the handle. */
void matchy_amd_extractor_set_unique(matchy_extractor_t *extractor, bool enabled);
bool matchy_amd_extractor_unique(const matchy_extractor_t *extractor);
void matchy_amd_extractor_reset_unique(matchy_extractor_t *extractor);
uint64_t matchy_amd_extractor_unique_count(const matchy_extractor_t *extractor);
/* Candidates as text (`matchy extract --render-on-gpu`). The candidates of `data` are put into the order of `matchy extract` — by line,
 * then domain, IPv4, e-mail, IPv6, hashes, Bitcoin, Ethereum, Monero, then by start — and written as that command's output on the
 * GPU: one line per candidate with the raw bytes data[start, end), for addresses too (not the canonical value),
 *   json  {"type":"<name>","value":"<bytes>"}   with \ -> \\ and " -> \" and no other escape
 *   csv   <name>,"<bytes>"                      with " doubled (the header line is the caller's)
 *   text  <bytes>
 * <name> being matchy_item_type_name in lower case. No candidate record crosses the bus. With matchy_amd_extractor_set_unique the block
 * holds the first occurrences only: exactly the candidates matchy_extractor_extract_chunk would have returned. The block is pinned
 * host memory, BORROWED until the handle's next call; inputs above the piece size of a scan are cut at newlines, their blocks handed
 * out end to end and their counts summed. A status other than _OK hands out nothing (text NULL, counts zero); the call still returns
 * MATCHY_SUCCESS, and a batch that was _REFUSED has not touched the set of distinct texts: extract_chunk can take it. MATCHY_ERROR_INVALID_PARAM for a NULL handle or out, NULL data
 * with len > 0, or an unknown format. Like extract_chunk this serialises on the handle. */
#define MATCHY_AMD_EXTRACT_FORMAT_JSON 0
#define MATCHY_AMD_EXTRACT_FORMAT_CSV 1
#define MATCHY_AMD_EXTRACT_FORMAT_TEXT 2
#define MATCHY_AMD_EXTRACT_TEXT_OK 0
#define MATCHY_AMD_EXTRACT_TEXT_REFUSED 1    /* a launch of more than 2^30 bytes or 2^32 list entries: the order key does not hold it */
#define MATCHY_AMD_EXTRACT_TEXT_MISCOUNT 2   /* the candidate lists did not hold what the scan counted: the block is not valid */
typedef struct matchy_amd_extract_text_t {
  const uint8_t *text;           /* NULL when there is none */
  uint64_t text_len;
  uint64_t n_records;
  uint64_t by_type[12];          /* records per MATCHY_ITEM_TYPE_* */
  uint32_t status;               /* MATCHY_AMD_EXTRACT_TEXT_* */
  uint32_t reserved;
} matchy_amd_extract_text_t;
int32_t matchy_amd_extractor_extract_rendered(const matchy_extractor_t *extractor, const uint8_t *data, uintptr_t len,
                                              uint32_t format /* 0 json, 1 csv, 2 text */, matchy_amd_extract_text_t *out);
/* Of the last _extract_rendered (its last piece): device milliseconds of keys + sort, of the measure step, of the write step, and of the
 * block's device-to-host copy. */
void matchy_amd_extractor_get_render_timing(const matchy_extractor_t *extractor, float out_ms[4]);
/* Allocations of the pass's buffers since the handle was made: a call like the one before adds none. */
uint64_t matchy_amd_extractor_render_allocations(const matchy_extractor_t *extractor);
const char *matchy_amd_last_error(void);
/* Diagnostics: states of the flattened Aho-Corasick automaton on the handle's default device; 0 = the database has no glob
 * section or its automaton is walked node by node (flattened table above MATCHY_AMD_DFA_MAX_MB, default 8192), -1 = error. */
int32_t matchy_amd_ac_dfa_states(const matchy_t *db);
/* Diagnostics: 1 when the database's globs are all of the form *LITERAL with one common first byte ("*.evil.com" lists) and the
 * scan decides glob candidates from hashed suffixes of a name instead of walking the automaton; 0 otherwise, -1 = error. */
int32_t matchy_amd_suffix_filter(const matchy_t *db);
/* Page-locked host memory (hipHostMalloc): buffers a host fills with log data and hands to matchy_scanner_scan reach the device
 * by DMA at the bus rate without being pinned per call. `matchy match` reads its input files into such buffers. */
void *matchy_amd_pinned_alloc(size_t bytes);
void matchy_amd_pinned_free(void *ptr);
/* Pin / unpin host memory the caller owns (hipHostRegister; page-aligned ranges): what matchy_scanner_scan does per call for
 * pageable buffers, for hosts that want to do it ahead of the scan (e.g. on a reader thread). */
int32_t matchy_amd_host_register(const void *ptr, size_t bytes);
void matchy_amd_host_unregister(const void *ptr);
/* HIP devices visible to the process (0 when there is none); `matchy match --devices all` */
int32_t matchy_amd_device_count(void);
/* Host topology for multi-GPU scatter / gather (every GPU is fed from host memory over its own PCIe link, and on a
 * two-socket node the H2D rate depends on which socket the feeding thread runs on). NUMA node of a device's PCI function
 * (hipDeviceGetPCIBusId -> /sys/bus/pci/devices/<id>/numa_node; -1 = the platform does not say), and binding of the CALLING thread to
 * the CPUs of that node (sched_setaffinity within the PROCESS's affinity as it was when the library was loaded — not the thread's current
 * mask, which a creating thread may already have narrowed to another node; returns the CPUs it may run on afterwards, 0 = unchanged).
 * matchy_amd_numa_cpus is the mapping itself over any sysfs root (tests): CPUs near `pci_bus_id`, count returned, first `cap` stored. */
int32_t matchy_amd_device_numa_node(int32_t device);
int32_t matchy_amd_bind_thread_to_device(int32_t device);
int32_t matchy_amd_unbind_thread(void); /* back to the process's affinity at load time; CPUs afterwards, 0 = unchanged */
int32_t matchy_amd_numa_cpus(const char *sysfs_root, const char *pci_bus_id, int32_t *out_cpus, size_t cap);

/* ---- Multi-device scanner (additive). The reader -> workers -> ordered gather of the reference's process_files_parallel
 * (crates/matchy/src/processing/parallel.rs:494-505; workers :594-704) behind the C ABI: the host submits newline-aligned batches,
 * one worker thread per entry of `devices` (an entry may repeat: several batches of one GPU in flight) scans them with a scanner of
 * its own, bound to the NUMA node of its GPU, and the host takes the results back in SUBMISSION order. Line blocks are independent
 * and the database is replicated per device: no collective; counters are summed by the caller. */
typedef struct matchy_multi_scanner_t matchy_multi_scanner_t;
typedef struct matchy_multi_batch_t {
  size_t seq;                  /* submission index */
  int32_t status;              /* MATCHY_SUCCESS or the error of this batch (text: matchy_amd_last_error) */
  matchy_scan_result_t result; /* canonical order, offsets relative to `data`; owned by the taker: matchy_scan_result_free */
  const uint8_t *data;
  size_t len;
  void *tag;                   /* as submitted (matchy_multi_scanner_scan_file: the batch's offset in the file) */
  void *payload;               /* what the batch hook returned for this batch, or NULL */
  size_t worker;               /* index into the device list of the worker that scanned it */
} matchy_multi_batch_t;
typedef struct matchy_multi_totals_t { uint64_t batches, bytes, lines, candidates, matches; } matchy_multi_totals_t;
/* Called on the WORKER thread right after a batch's scan (per-hit work such as rendering runs in parallel there); the
 * returned pointer travels with the batch as matchy_multi_batch_t.payload. */
typedef void *(*matchy_multi_batch_fn)(void *user, size_t worker, matchy_scanner_t *scanner, const matchy_scan_result_t *result,
                                       const uint8_t *data, size_t len, void *tag);
/* Called on the gathering thread, batches in order; non-zero stops the scan and is returned. */
typedef int32_t (*matchy_multi_ordered_fn)(void *user, const matchy_multi_batch_t *batch);
/* devices NULL / n_devices 0 = the handle's default device once. extract_flags as matchy_scanner_create. NULL on failure. */
matchy_multi_scanner_t *matchy_multi_scanner_create(const matchy_t *db, uint32_t extract_flags, const int32_t *devices, size_t n_devices);
void matchy_multi_scanner_free(matchy_multi_scanner_t *ms);
size_t matchy_multi_scanner_workers(const matchy_multi_scanner_t *ms);
/* The scanner of a worker (NULL until that worker has seen a batch; worker 0's exists from the start): for matchy_scan_hit_to_json /
 * matchy_scan_result_to_ndjson of a batch that worker scanned (use it from one thread at a time). */
matchy_scanner_t *matchy_multi_scanner_worker_scanner(const matchy_multi_scanner_t *ms, size_t worker);
void matchy_multi_scanner_set_batch_hook(matchy_multi_scanner_t *ms, matchy_multi_batch_fn fn, void *user);
/* Queue one batch (it should end at a line end; len < 4 GiB). The bytes stay the caller's and must remain valid until the batch has
 * been taken with _next. BACK-PRESSURE (the reference's bounded channels, processing/parallel.rs:563-577): blocks while one batch
 * per worker is already waiting, and while matchy_multi_scanner_max_pending() batches (2 x workers + 2) are out — submitted and not
 * yet taken with _next, finished or not. Submit from one thread and gather from another, or interleave on one thread: call _next
 * whenever matchy_multi_scanner_pending() has reached the maximum (a lone thread that only submits would block for good).
 * pinned_range: NULL, or the page range the caller registered for this batch with matchy_amd_host_register — the worker unregisters it
 * after the scan (if submit FAILS the range is still the caller's to unregister). */
int32_t matchy_multi_scanner_submit(matchy_multi_scanner_t *ms, const uint8_t *data, size_t len, void *tag, const void *pinned_range);
/* The same with the NUMA node the batch's bytes live on (-1 = anywhere = matchy_multi_scanner_submit): a worker whose GPU hangs off
 * that node takes it first, a worker of another node only when it has nothing of its own. */
int32_t matchy_multi_scanner_submit_near(matchy_multi_scanner_t *ms, const uint8_t *data, size_t len, void *tag, const void *pinned_range,
                                         int32_t numa_node);
/* matchy_multi_scanner_submit of a batch of n segments (matchy_scanner_set_segments: `starts` is copied): the worker that takes the
 * batch sets the table on its scanner before the scan, and the batch from _next answers matchy_scan_result_segments. */
int32_t matchy_multi_scanner_submit_segments(matchy_multi_scanner_t *ms, const uint8_t *data, size_t len, const uint32_t *starts, size_t n,
                                             void *tag, const void *pinned_range);
/* matchy_multi_scanner_submit of a pack of n gzip files (matchy_scanner_scan_gz: `members` is copied, the packed bytes stay the
 * caller's until the batch has been taken): the worker that takes the batch inflates and scans it on its GPU. The batch from _next
 * answers matchy_scan_result_segments and matchy_scan_result_gz; its data / len are the inflated text, owned by the result, and its
 * length — NULL and the length without want_text. */
int32_t matchy_multi_scanner_submit_gz(matchy_multi_scanner_t *ms, const uint8_t *packed, size_t packed_len, const matchy_gz_member_t *members,
                                       size_t n, bool want_text, void *tag);
/* The same for a pack of n_files gzip files of one member or many (matchy_scanner_scan_gz_files: `files` is copied). The batch from
 * _next answers matchy_scan_result_gz_files as well. */
int32_t matchy_multi_scanner_submit_gz_files(matchy_multi_scanner_t *ms, const uint8_t *packed, size_t packed_len, const matchy_gz_file_t *files,
                                             size_t n_files, bool want_text, void *tag);
/* The same for one window of a large multi-member file (matchy_scanner_scan_gz_window: the carry is copied at the call, the packed
 * bytes stay the caller's). The batch from _next answers matchy_scan_result_gz_window as well. The windows of one file are serial: the
 * caller takes a window's batch, and with it the carry, before it submits the next. */
int32_t matchy_multi_scanner_submit_gz_window(matchy_multi_scanner_t *ms, const uint8_t *packed, size_t packed_len, const matchy_gz_window_t *window,
                                              bool want_text, void *tag);
/* The same for one window of one large DEFLATE stream (matchy_scanner_scan_gz_stream: state and carry are copied at the call, the packed
 * bytes stay the caller's; matchy_multi_scanner_set_gz_pieces must be on, else the batch comes back with MATCHY_ERROR_INVALID_PARAM). The
 * batch from _next answers matchy_scan_result_gz_stream as well. The windows of one stream are serial: submit one, take it, submit the next. */
int32_t matchy_multi_scanner_submit_gz_stream(matchy_multi_scanner_t *ms, const uint8_t *packed, size_t packed_len, const matchy_gz_stream_window_t *window,
                                              bool want_text, void *tag);
/* matchy_scanner_set_gz_pieces for every worker: each sets its scanner to the value in front of a gz batch it takes. */
int32_t matchy_multi_scanner_set_gz_pieces(matchy_multi_scanner_t *ms, uint32_t piece_bytes);
/* NUMA node of a worker's GPU (-1 = unknown) and the number of CPUs its thread bound itself to (0 = not bound); valid once the
 * worker thread has started (after the first _next at the latest). */
int32_t matchy_multi_scanner_worker_numa(const matchy_multi_scanner_t *ms, size_t worker, int32_t *node, int32_t *cpus_bound);
size_t matchy_multi_scanner_pending(const matchy_multi_scanner_t *ms);     /* submitted and not yet taken */
size_t matchy_multi_scanner_max_pending(const matchy_multi_scanner_t *ms); /* the bound submit blocks on */
/* The next batch in submission order (blocks until it is done): 1 = *out filled, 0 = nothing pending, < 0 = error. */
int32_t matchy_multi_scanner_next(matchy_multi_scanner_t *ms, matchy_multi_batch_t *out);
/* One buffer through all workers, cut at newlines into pieces of batch_bytes (0 = chosen from len and the worker count), merged into
 * ONE result with offsets into `data`: the same records matchy_scanner_scan returns for these bytes, whatever the device list. */
int32_t matchy_multi_scanner_scan(matchy_multi_scanner_t *ms, const uint8_t *data, size_t len, size_t batch_bytes, matchy_scan_result_t *out);
/* One input file: a regular file is mapped (its batches are cut, pre-faulted and pinned by a reader thread), "-" / a pipe is read.
 * `fn` (may be NULL) sees every batch in file order on the calling thread, tag = offset of the batch in the input; totals may be NULL. */
int32_t matchy_multi_scanner_scan_file(matchy_multi_scanner_t *ms, const char *path, size_t batch_bytes, matchy_multi_ordered_fn fn,
                                       void *user, matchy_multi_totals_t *totals);
/* Line context for the scanner of every worker (from the next batch a worker takes). Batches from _next carry values relative to
 * their batch; matchy_multi_scanner_scan merges them into values relative to `data`, like matchy_scanner_scan. */
void matchy_multi_scanner_set_line_context(matchy_multi_scanner_t *ms, bool enabled);
/* Hit lines for the scanner of every worker (from the next batch a worker takes). Batches from _next answer
 * matchy_scan_result_hit_lines (and _lines), owned by the result, and render with text == NULL — a gz batch submitted without want_text
 * included, whose `data` is NULL. The merged results of matchy_multi_scanner_scan / _scan_file do not carry the block. */
void matchy_multi_scanner_set_hit_lines(matchy_multi_scanner_t *ms, bool enabled);
/* Rendered records (matchy_scanner_set_render) on the multi-device scanner: arms the NEXT batch submitted (matchy_multi_scanner_submit / _submit_near / _submit_segments / _submit_gz / _submit_gz_files;
 * copied at the call, NULL disarms). The worker that takes the batch arms its scanner; the batch's result owns the block. An armed gz
 * batch submitted without want_text is scanned with line context whatever matchy_multi_scanner_set_line_context says: its result carries
 * the lines with matches per segment, which nobody could count from a text that does not come back. A batch whose
 * parameters do not fit it comes back with MATCHY_ERROR_INVALID_PARAM in its status, like any batch that failed. */
int32_t matchy_multi_scanner_set_render(matchy_multi_scanner_t *scanner, const matchy_render_params_t *params);

/* ---- Hit tally (opt-in, off by default: with it never enabled a scanner allocates, launches and copies nothing more and every output
 * stays as it is). How often every distinct matched value hit: a table in device memory, owned by the scanner, keyed by (item type,
 * matched text) — the raw bytes data[start, start + length) of a hit record, case-sensitive, not NUL-terminated; for IP addresses the
 * text in the log — fed from the hit records of every lookup scan while its batch is still resident, whatever the entry and the fetch
 * mode (counts only, records, sorted, device-resident, compact), kept across scans, and read out as a top-N list: only counters and the
 * rows of the report cross the bus. Pattern ids are deliberately not the key: `pattern_ids` mixes literal and glob ids, which both start
 * at 0, and many networks share one data offset; matchy_amd_query_json(text) gives a reported value's cidr / data / patterns back.
 * _set_tally applies from the next scan; switching it off keeps what was counted, _reset_tally empties it (and keeps its allocations),
 * matchy_scanner_free releases it. A NULL handle is harmless. */
void matchy_scanner_set_tally(matchy_scanner_t *scanner, bool enabled);
bool matchy_scanner_tally(const matchy_scanner_t *scanner);
void matchy_scanner_reset_tally(matchy_scanner_t *scanner);
typedef struct matchy_tally_entry_t { const uint8_t *text; uint32_t len; uint8_t item_type; uint64_t count; } matchy_tally_entry_t;
typedef struct matchy_tally_t { const matchy_tally_entry_t *entries; size_t n_entries; uint64_t distinct, matches; void *_internal; } matchy_tally_t;
/* The first `limit` entries (0 = all) ordered by count descending, then by the extractor order of the type (IPv6, IPv4, e-mail, domain,
 * hashes, Bitcoin, Ethereum, Monero), then by text bytewise ascending; `distinct` = entries in the table, `matches` = hits counted (the
 * sum of all counts). The selection is made from the counts; only the texts of the chosen entries are copied back. Release with
 * matchy_tally_free. MATCHY_ERROR_INVALID_PARAM for a scanner that never enabled the tally. */
int32_t matchy_scanner_tally_top(matchy_scanner_t *scanner, size_t limit, matchy_tally_t *out);
/* The same for every worker's scanner of a multi-device scanner: _set_tally applies from the next batch a worker takes. _tally_top
 * and _reset_tally need matchy_multi_scanner_pending() == 0 (MATCHY_ERROR_INVALID_PARAM otherwise; _reset_tally then does nothing):
 * _tally_top exports every worker's whole table, merges by (type, text) on the host, then orders and cuts. */
int32_t matchy_multi_scanner_set_tally(matchy_multi_scanner_t *ms, bool enabled);
int32_t matchy_multi_scanner_tally_top(matchy_multi_scanner_t *ms, size_t limit, matchy_tally_t *out);
void matchy_multi_scanner_reset_tally(matchy_multi_scanner_t *ms);
void matchy_tally_free(matchy_tally_t *tally);

/* ---- Whole-line queries (opt-in, off by default: with it never enabled a scanner allocates, launches and copies nothing more and every
 * output stays as it is). While on, a lookup scan — matchy_scanner_scan, _scan_device, _submit_device / _wait and the multi-device
 * scanner's entries — treats its buffer as a LIST OF QUERIES instead of log text, and answers every line like matchy_query answers one
 * value (Database::lookup without the cache). Extraction, the extract flags of the scanner and the label rules play no part.
 *   Lines are cut at '\n'; a final piece without '\n' is a line; a buffer that ends in '\n' has no empty line behind it; len == 0 has none.
 *   The query is the line without exactly one trailing '\r'. Nothing else is trimmed; an empty line is a query.
 *   A query the IP address parser accepts as a whole (IPv4, IPv6, IPv6 with an embedded dotted quad; no zone, no prefix length) walks the
 *   tree, IPv4 in an IPv6 tree from its IPv4 start node. Anything else takes the string path: literal table, then every glob over the
 *   whole query, with the case folding of the database. A query that is not valid UTF-8 is not looked up and is counted.
 *   A found query is ONE ordinary hit record: start / length = the query inside the buffer (without the '\r'); kind, prefix, value and
 *   ids as the single query reports them; item type MATCHY_ITEM_TYPE_IPV4 / _IPV6 for addresses and _DOMAIN for strings. A sorted fetch
 *   is in line order, `lines` stays the number of '\n' bytes, `candidates` counts the queries that were looked up.
 *   A query of 16 MiB or more, or more than 65535 glob ids on one query, fail the scan as they do without the mode.
 * Works with sorted fetches, line context (`line` is the 0-based index of the query), the hit tally (hits per distinct query text) and the
 * multi-device scanner. NOT combined with segments, gz scans, hit lines or rendered records: a scan that finds one of them set together
 * with the mode launches nothing and returns MATCHY_ERROR_INVALID_PARAM, matchy_amd_last_error() names the pair, and a pending segment
 * table or render parameters are dropped. The scan runs on one stream: matchy_scanner_set_slices has no effect on it. */
void matchy_scanner_set_whole_lines(matchy_scanner_t *scanner, bool enabled);
bool matchy_scanner_whole_lines(const matchy_scanner_t *scanner);
/* queries, address queries, string queries and queries that are not valid UTF-8 of the last scan in the mode (matchy_scanner_scan: summed
 * over its pieces) */
void matchy_scanner_get_whole_lines_counters(const matchy_scanner_t *scanner, uint64_t out[4]);
/* With matchy_scanner_set_profile: milliseconds of count + prefix, of scatter + classify, and of the lookups of the last scan in the mode. */
void matchy_scanner_get_whole_lines_timing(const matchy_scanner_t *scanner, float out_ms[3]);
/* The mode for every worker's scanner; needs matchy_multi_scanner_pending() == 0 (MATCHY_ERROR_INVALID_PARAM otherwise). */
int32_t matchy_multi_scanner_set_whole_lines(matchy_multi_scanner_t *ms, bool enabled);

/* ---- UTF-16 inputs (opt-in: with these calls never made a scanner allocates, launches and copies nothing more and every output stays
 * as it is). `data` — host or device memory — is `len` bytes of UTF-16 in the given byte order; it is transcoded to UTF-8 on the GPU
 * (count, prefix, write: three passes over the batch and one 16-byte read of the text's length) and the ordinary lookup scan runs over
 * the UTF-8 text on the same stream.
 *   len / 2 code units; a surrogate pair becomes the 4 bytes of its code point; every unpaired surrogate and an odd last byte become
 *   EF BF BD (U+FFFD) each — Rust's String::from_utf16_lossy, with one more U+FFFD for the odd byte. CPython's codec differs in one
 *   place: it writes ONE U+FFFD for a high surrogate followed by an odd last byte, this call writes two.
 *   No BOM handling: the bytes handed in are transcoded, U+FEFF becomes EF BB BF and U+FFFE becomes EF BF BE. Skip a BOM before the call.
 * Every fetch mode of matchy_scanner_scan_device, line context, hit lines, rendered records and the tally work as they do there:
 * `bytes` is the length of the UTF-8 text, `lines` counts its '\n' bytes and the offsets of hits and line records are offsets into it.
 * want_text: the UTF-8 batch is copied to pinned host memory once, behind the scan, for matchy_scan_hit_to_json and the NDJSON calls.
 * NOT combined with segments or whole-line queries. MATCHY_ERROR_INVALID_PARAM with a message, and a scanner that stays usable: NULL
 * handles, byte_order above 1, an input whose bound 3 * (len / 2) + 3 * (len & 1) reaches 2^31, a pending segment table (dropped) and
 * whole-line mode. */
#define MATCHY_UTF16_LE 0u
#define MATCHY_UTF16_BE 1u
int32_t matchy_scanner_scan_utf16(matchy_scanner_t *scanner, const uint8_t *data, size_t len, uint32_t byte_order, uint32_t fetch_mode,
                                  bool want_text, matchy_scan_result_t *out);
/* text / text_len: the UTF-8 batch — NULL / its length without want_text; borrowed from the scanner until its next scan, or owned by
 * the result for MATCHY_SCAN_FETCH_SORTED (like the hit arrays of that mode). code_units: len / 2. replaced: U+FFFD written.
 * MATCHY_ERROR_INVALID_PARAM for a result of another kind of scan. Any out pointer may be NULL. */
int32_t matchy_scan_result_utf16(const matchy_scan_result_t *result, const uint8_t **text, size_t *text_len, uint64_t *code_units,
                                 uint64_t *replaced);
/* Milliseconds of the count, prefix and write steps of the last UTF-16 scan (recorded for every such scan, with or without
 * matchy_scanner_set_profile: four event records per batch); zeros before the first. */
void matchy_scanner_get_utf16_timing(const matchy_scanner_t *scanner, float out_ms[3]);
/* Input bytes per tile of the passes, and tiles per workgroup of the prefix step (tests place their cases on these boundaries). */
void matchy_amd_utf16_geometry(uint32_t out[2]);
/* matchy_multi_scanner_submit of a UTF-16 batch: the worker that takes it transcodes and scans it on its GPU. The batch from _next
 * answers matchy_scan_result_utf16; its data / len are the UTF-8 text, owned by the result, and its length — NULL and the length
 * without want_text. pinned_range as for matchy_multi_scanner_submit. A batch armed with matchy_multi_scanner_set_render that is
 * submitted without want_text is scanned with line context whatever the setting is, like an armed gz pack. */
int32_t matchy_multi_scanner_submit_utf16(matchy_multi_scanner_t *ms, const uint8_t *data, size_t len, uint32_t byte_order, bool want_text,
                                          void *tag, const void *pinned_range);
/* ---- Percent- and JSON-escaped inputs (opt-in: with these calls never made a scanner allocates, launches and copies nothing more and
 * every output stays as it is). `data` — host or device memory — is `len` bytes of text that carries escapes; it is decoded on the GPU
 * (count, prefix, write over the batch and one 16-byte read of the text's length; JSON: a scan over the tiles for the escape state in
 * front of them) and the ordinary lookup scan runs over the decoded text on the same stream. modes: MATCHY_UNESCAPE_PERCENT,
 * MATCHY_UNESCAPE_JSON, or both: then the text is percent(json(data)), two runs of the pass.
 * Every input position emits 0 to 4 bytes. The bytes of a valid escape are consumed: its first byte owns the output.
 *   PERCENT  '%' followed by two hex digits (either case), all inside the input: the byte with that value. Anything else is literal,
 *            '%' with fewer than two hex digits behind it or at the end of the input included. '+' stays '+'; "%25" becomes '%' once:
 *            one pass, no re-scan of its output.
 *   JSON     A backslash is an introducer if it is not itself escaped: esc[i] = data[i-1] == '\\' && !esc[i-1], esc[0] = 0.
 *            An introducer and one of " \ / b f n r t: a two-byte escape for the byte it names. An introducer, 'u' and four hex
 *            digits: a six-byte escape for a UTF-16 code unit, written as UTF-8. A high-surrogate escape followed immediately by a
 *            low-surrogate escape is written as the four bytes of the pair (the low one emits nothing); any other surrogate escape as
 *            EF BF BD, one per escape. An introducer followed by anything else is NOT an escape and both bytes emit themselves (\u
 *            with fewer than four hex digits, a backslash in front of a real LF or as the last byte); the byte behind it still counts
 *            as escaped.
 *   Line ends, both modes: a real 0x0A always emits itself. An escape whose value is LF (%0A, %0a, \n, \u000a, \u000A) is written as
 *            ONE SPACE: a boundary byte for every extractor that LF is one for, but it ends no line. The decoded text has exactly the
 *            LF bytes of the input, in order, and since no escape spans a real LF, decode(A + B) == decode(A) + decode(B) for any
 *            cut behind an LF: batches cut at line ends need no state from the batch before.
 * The text is never longer than the input. Every fetch mode of matchy_scanner_scan_device, line context, hit lines, rendered records
 * and the tally work as they do there: `bytes` is the length of the decoded text, `lines` counts its '\n' bytes and the offsets of hits
 * and line records are offsets into it (no mapping back to the raw input).
 * want_text: the decoded batch is copied to pinned host memory once, behind the scan, for matchy_scan_hit_to_json and the NDJSON calls.
 * NOT combined with segments or whole-line queries. MATCHY_ERROR_INVALID_PARAM with a message, and a scanner that stays usable: NULL
 * handles, modes 0 or above 3, no input, len >= 0x7FFF0000, a pending segment table (dropped) and whole-line mode. */
#define MATCHY_UNESCAPE_PERCENT 1u
#define MATCHY_UNESCAPE_JSON 2u
int32_t matchy_scanner_scan_escaped(matchy_scanner_t *scanner, const uint8_t *data, size_t len, uint32_t modes, uint32_t fetch_mode,
                                    bool want_text, matchy_scan_result_t *out);
/* text / text_len: the decoded batch — NULL / its length without want_text; borrowed from the scanner until its next scan, or owned by
 * the result for MATCHY_SCAN_FETCH_SORTED (like the hit arrays of that mode). counters: valid escapes decoded, U+FFFD written, escapes
 * for LF written as a space; with both modes, summed over the two runs. MATCHY_ERROR_INVALID_PARAM for a result of another kind of
 * scan. Any out pointer may be NULL. */
int32_t matchy_scan_result_unescaped(const matchy_scan_result_t *result, const uint8_t **text, size_t *text_len, uint64_t counters[3]);
/* Milliseconds of the count (JSON: with the state steps), prefix and write steps of the last escaped scan, summed over its runs
 * (recorded for every such scan, with or without matchy_scanner_set_profile); zeros before the first. */
void matchy_scanner_get_unescape_timing(const matchy_scanner_t *scanner, float out_ms[3]);
/* Input bytes per tile of the passes, tiles per workgroup of the prefix step, tiles per workgroup of the state scan (tests place
 * their cases on these boundaries). */
void matchy_amd_unescape_geometry(uint32_t out[3]);
/* matchy_multi_scanner_submit of an escaped batch: the worker that takes it decodes and scans it on its GPU. The batch from _next
 * answers matchy_scan_result_unescaped; its data / len are the decoded text, owned by the result, and its length — NULL and the length
 * without want_text. pinned_range as for matchy_multi_scanner_submit. A batch armed with matchy_multi_scanner_set_render that is
 * submitted without want_text is scanned with line context whatever the setting is, like an armed gz pack. */
int32_t matchy_multi_scanner_submit_escaped(matchy_multi_scanner_t *ms, const uint8_t *data, size_t len, uint32_t modes, bool want_text,
                                            void *tag, const void *pinned_range);
/* Deterministic builds for tests: fixes the build_epoch metadata value. */
int32_t matchy_builder_set_build_epoch(matchy_builder_t *b, uint64_t epoch);

#ifdef __cplusplus
}
#endif
#endif /* MATCHY_AMD_H */
