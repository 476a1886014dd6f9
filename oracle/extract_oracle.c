/*
 * extract_oracle.c -- CPU ORACLE for the off-target extraction step.
 *
 * TEST INFRASTRUCTURE, NOT PRODUCT CODE (only tests/ and measurement scripts may use it).
 * Restates /root/reference/src/crackling/utils/extractOfftargets.py:
 *   :23-24   the two lookahead patterns  [ACG][ACGT]{19}[ACGT][AG]G   and   C[CT][ACGT][ACGT]{19}[TGC]
 *   :97-110  every (overlapping) match contributes the first 20 characters of the 23-character match -- as they
 *            are on the forward pattern, reverse-complemented (Helpers.py:7-10) on the reverse pattern
 *   :112-191 all sites, one per line, sorted (duplicates kept)
 * Files are read in Python's text mode: "\n", "\r\n" and a lone "\r" each end a line.  Blanks are what str.strip()
 * removes from ASCII text: space, \t \n \v \f \r and the separators 0x1c-0x1f.
 *
 * ONE input (n_files == 1; :209-222, explodeMultiFastaFile :26-62): every line is stripped; a stripped line starting
 * with '>' opens a record; other lines are upper-cased and concatenated.
 *
 * SEVERAL inputs (n_files > 1; processingNode :74-90 on each file as it is): a line is a header when its first RAW
 * character is '>'; other lines lose their trailing blanks only (rstrip) -- leading blanks, and so a header line
 * with blanks before the '>', are sequence text -- and are upper-cased and concatenated.  The records of one file are
 * keyed by the header line (the text behind '>' with its line end, which text mode makes "\n" -- or without one when
 * the header is the last line of a file that does not end in a line end): a repeated header empties the record before
 * it (:83-85), so only the last record under a key counts.  Keys of different files do not meet.  Lines before the
 * first header form a record of their own (keyed by the file's path: never equal to a header key here).
 *
 * Where the reference raises, this oracle -- like the product -- carries on (n_files == 1 only):
 *   a blank line            IndexError at :36          -> skipped
 *   sequence before the first header
 *                           AttributeError at :56      -> a record of its own
 * Pinned by tests/golden/extract/ (made by oracle/make_golden_extract.py and oracle/make_golden_extract_cases.py from
 * that Python code; cases.json records the two rejected inputs and this oracle's line counts for them).
 */
#include <ctype.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static int is_acgt(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

static int cmp20(const void *a, const void *b) { return memcmp(a, b, 20); }

static void scan_record(const char *s, size_t n, char **out, size_t *cnt, size_t *cap)
{
    for (size_t i = 0; i + 23 <= n; i++) {
        int body = 1;
        for (int k = 1; k <= 20 && body; k++) body = is_acgt(s[i + k]); /* chars 1..20 are [ACGT] in both patterns */
        if (!body) continue;
        /* forward: [ACG] [ACGT]{19} [ACGT] [AG] G */
        int fwd = (s[i] == 'A' || s[i] == 'C' || s[i] == 'G') && (s[i + 21] == 'A' || s[i + 21] == 'G') && s[i + 22] == 'G';
        /* reverse: C [CT] [ACGT] [ACGT]{19} [TGC] */
        int rev = s[i] == 'C' && (s[i + 1] == 'C' || s[i + 1] == 'T') && is_acgt(s[i + 21]) &&
                  (s[i + 22] == 'T' || s[i + 22] == 'G' || s[i + 22] == 'C');
        for (int pass = 0; pass < 2; pass++) {
            if (!(pass == 0 ? fwd : rev)) continue;
            if (*cnt == *cap) {
                *cap = *cap ? *cap * 2 : 1024;
                *out = (char *)realloc(*out, *cap * 20);
            }
            char *dst = *out + *cnt * 20;
            if (pass == 0) {
                memcpy(dst, s + i, 20);
            } else {
                for (int k = 0; k < 20; k++) {
                    char c = s[i + 19 - k];
                    dst[k] = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
                }
            }
            (*cnt)++;
        }
    }
}

static int py_blank(char c) { return c == ' ' || (c >= '\t' && c <= '\r') || (c >= 0x1c && c <= 0x1f); }

/* Line [p, *e) of text mode and the start of the next one. */
static size_t next_line(const char *s, size_t len, size_t p, size_t *e, int *ended)
{
    size_t q = p;
    while (q < len && s[q] != '\n' && s[q] != '\r') q++;
    *e = q;
    *ended = q < len;
    if (q < len && s[q] == '\r' && q + 1 < len && s[q + 1] == '\n') q++;
    return q < len ? q + 1 : len;
}

/* One input: explode rules. */
static void scan_single(const char *fasta, size_t len, char **sites, size_t *cnt, size_t *cap)
{
    char *seq = (char *)malloc(len + 1);
    size_t n = 0, p = 0;
    while (p < len) {
        size_t e;
        int ended;
        size_t next = next_line(fasta, len, p, &e, &ended);
        size_t a = p, b = e;
        while (a < b && py_blank(fasta[a])) a++;
        while (b > a && py_blank(fasta[b - 1])) b--;
        if (b > a && fasta[a] == '>') { /* new record */
            scan_record(seq, n, sites, cnt, cap);
            n = 0;
        } else {
            for (size_t k = a; k < b; k++) seq[n++] = (char)toupper((unsigned char)fasta[k]);
        }
        p = next;
    }
    scan_record(seq, n, sites, cnt, cap);
    free(seq);
}

/* Several inputs: one file by the per-file rules. */
typedef struct {
    const char *hdr;   /* header text behind '>' (NULL: the lines before the first header) */
    size_t hdr_len;
    int ended;         /* the header line has a line end */
    size_t seq_at, seq_len;
    size_t order;
} record;

static int cmp_record(const void *x, const void *y)
{
    const record *a = (const record *)x, *b = (const record *)y;
    if (!a->hdr != !b->hdr) return a->hdr ? 1 : -1;
    if (a->hdr) {
        size_t m = a->hdr_len < b->hdr_len ? a->hdr_len : b->hdr_len;
        int c = memcmp(a->hdr, b->hdr, m);
        if (c) return c;
        if (a->hdr_len != b->hdr_len) return a->hdr_len < b->hdr_len ? -1 : 1;
        if (a->ended != b->ended) return a->ended - b->ended;
    }
    return a->order < b->order ? -1 : a->order > b->order;
}

static void scan_whole_file(const char *fasta, size_t len, char **sites, size_t *cnt, size_t *cap)
{
    char *seq = (char *)malloc(len + 1);
    size_t n = 0, p = 0, n_rec = 1, cap_rec = 16;
    record *recs = (record *)malloc(cap_rec * sizeof(record));
    recs[0] = (record){NULL, 0, 0, 0, 0, 0};
    while (p < len) {
        size_t e;
        int ended;
        size_t next = next_line(fasta, len, p, &e, &ended);
        if (fasta[p] == '>') {
            recs[n_rec - 1].seq_len = n - recs[n_rec - 1].seq_at;
            if (n_rec == cap_rec) recs = (record *)realloc(recs, (cap_rec *= 2) * sizeof(record));
            recs[n_rec] = (record){fasta + p + 1, e - p - 1, ended, n, 0, n_rec};
            n_rec++;
        } else {
            size_t b = e;
            while (b > p && py_blank(fasta[b - 1])) b--;
            for (size_t k = p; k < b; k++) seq[n++] = (char)toupper((unsigned char)fasta[k]);
        }
        p = next;
    }
    recs[n_rec - 1].seq_len = n - recs[n_rec - 1].seq_at;
    qsort(recs, n_rec, sizeof(record), cmp_record);
    for (size_t r = 0; r < n_rec; r++) {
        /* the last record under a key: the next one in (key, order) order has another key */
        if (r + 1 < n_rec) {
            record next = recs[r + 1];
            next.order = recs[r].order;
            if (cmp_record(&recs[r], &next) == 0) continue;
        }
        scan_record(seq + recs[r].seq_at, recs[r].seq_len, sites, cnt, cap);
    }
    free(recs);
    free(seq);
}

/* Several files -> sorted text (20 chars + '\n' per site), malloc'd. */
char *oracle_extract(const char *const *files, const size_t *lens, int n_files, size_t *out_len)
{
    char *sites = NULL;
    size_t cnt = 0, cap = 0;
    for (int f = 0; f < n_files; f++) {
        if (n_files == 1) scan_single(files[f], lens[f], &sites, &cnt, &cap);
        else scan_whole_file(files[f], lens[f], &sites, &cnt, &cap);
    }
    qsort(sites, cnt, 20, cmp20);
    char *text = (char *)malloc(cnt * 21 + 1);
    for (size_t i = 0; i < cnt; i++) {
        memcpy(text + i * 21, sites + i * 20, 20);
        text[i * 21 + 20] = '\n';
    }
    free(sites);
    *out_len = cnt * 21;
    return text;
}

void oracle_extract_free(void *p) { free(p); }
