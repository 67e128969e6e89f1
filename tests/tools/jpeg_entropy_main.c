/* Stand-alone driver of cerberus_amd/csrc/jpeg_entropy.h for the host sanitizers (tests/test_jpeg_host.py compiles it with
 * -fsanitize=address,undefined and runs it as a child process; nothing sanitised is ever loaded into Python).
 *
 *     jpeg_entropy_main <directory>
 *
 * Every file `*.jpg` of the directory is decoded whole (a file `<name>.tables` beside it is its JPEGTables stream), then at 16 seeded prefix
 * truncations and with 64 seeded single-byte corruptions.  Every input lives in a heap block of EXACTLY its size and the coefficients in one of exactly
 * the size the intact stream needs, so a read past n_src or a write past coef_cap is a sanitizer report.  Exit status 0: every call returned one of the
 * four defined codes and every intact stream decoded. */
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../cerberus_amd/csrc/jpeg_entropy.h"

static uint8_t* slurp(const char* path, int64_t* n) {
    FILE* f = fopen(path, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    *n = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* b = (uint8_t*)malloc(*n > 0 ? (size_t)*n : 1);
    if (b && fread(b, 1, (size_t)*n, f) != (size_t)*n) {
        free(b);
        b = NULL;
    }
    fclose(f);
    return b;
}

static uint32_t lcg(uint32_t* s) {
    *s = *s * 1664525u + 1013904223u;
    return *s >> 8;
}

static int defined_code(int rc) { return rc == CERB_JPEG_OK || rc == CERB_JPEG_UNSUPPORTED || rc == CERB_JPEG_CORRUPT || rc == CERB_JPEG_TOO_LARGE; }

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    DIR* d = opendir(argv[1]);
    if (!d) return 2;
    struct dirent* e;
    int files = 0, calls = 0;
    uint32_t seed = 12345u;
    while ((e = readdir(d)) != NULL) {
        const size_t ln = strlen(e->d_name);
        if (ln < 5 || strcmp(e->d_name + ln - 4, ".jpg") != 0) continue;
        char path[4096], tpath[4200];
        snprintf(path, sizeof(path), "%s/%s", argv[1], e->d_name);
        snprintf(tpath, sizeof(tpath), "%s.tables", path);
        int64_t n = 0, nt = 0;
        uint8_t* src = slurp(path, &n);
        uint8_t* tab = slurp(tpath, &nt);
        if (!src) return 3;
        cerb_jpeg_state st;
        cerb_jpeg_hdr hdr;
        int64_t scan = 0, used = 0;
        int rc = cerb_jpeg_parse_tile(&st, tab, nt, src, n, &scan);
        int64_t cap = rc == CERB_JPEG_OK ? cerb_jpeg_fill_hdr(&st, 0, &hdr) : 0;
        int16_t* coefs = (int16_t*)malloc(cap > 0 ? (size_t)cap * sizeof(int16_t) : 1);
        const int whole = cerb_jpeg_entropy_decode(tab, nt, src, n, 0, &hdr, coefs, cap, &used);
        ++calls;
        if (!defined_code(whole) || whole == CERB_JPEG_CORRUPT || whole == CERB_JPEG_TOO_LARGE || (whole == CERB_JPEG_OK && used != cap)) {
            fprintf(stderr, "%s: intact stream -> %d (%lld of %lld coefficients)\n", path, whole, (long long)used, (long long)cap);
            return 1;
        }
        for (int k = 0; k < 16 + 64; ++k) {
            int64_t m = n;
            if (k < 16) m = (int64_t)(lcg(&seed) % (uint32_t)(n > 0 ? n : 1));
            uint8_t* cut = (uint8_t*)malloc(m > 0 ? (size_t)m : 1);
            memcpy(cut, src, (size_t)m);
            if (k >= 16 && m > 0) cut[lcg(&seed) % (uint32_t)m] ^= (uint8_t)(1 + lcg(&seed) % 255);
            rc = cerb_jpeg_entropy_decode(tab, nt, cut, m, k & 1, &hdr, coefs, cap, &used);
            ++calls;
            free(cut);
            if (!defined_code(rc) || used > cap || (k < 16 && rc == CERB_JPEG_OK && whole != CERB_JPEG_OK)) {
                fprintf(stderr, "%s: variant %d -> %d\n", path, k, rc);
                return 1;
            }
        }
        free(coefs);
        free(src);
        free(tab);
        ++files;
    }
    closedir(d);
    printf("%d files, %d calls\n", files, calls);
    return files > 0 ? 0 : 4;
}
