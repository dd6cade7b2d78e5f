/* The oracle's dictionary finalize (oracle/zso_encoder.c: zso_trainStats, zso_finalizeDictionary) and the trainer's scalar model
 * (train_model.c: model_train) driven outside Python, so that a read or write past an input or an output is the address sanitizer's to see:
 * the samples, the sizes, the content and the dictionary each lie in a heap block of exactly their size.
 * tests/test_dict_finalize_host.py builds it with -fsanitize=address,undefined and holds the lines and files against the library's answers.
 *
 *   dict_finalize (SAMPLES SIZES CAP K D F OUT)...
 * SAMPLES: the samples back to back; SIZES: their sizes as text; OUT: where the dictionary goes.  One line an input:
 *   <content bytes> <dictionary bytes> <literals counted> <sequences counted> */
#include "zso_oracle.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

size_t model_train(const uint8_t *samples, const size_t *sizes, unsigned n, uint8_t *dict, size_t cap, unsigned k, unsigned d, unsigned f);

static uint8_t *slurp(const char *path, size_t *size)
{
    FILE *fp = fopen(path, "rb");
    long n;
    uint8_t *p;
    if (!fp) { perror(path); exit(2); }
    fseek(fp, 0, SEEK_END); n = ftell(fp); fseek(fp, 0, SEEK_SET);
    p = (uint8_t *)malloc(n ? (size_t)n : 1);
    if (n && fread(p, 1, (size_t)n, fp) != (size_t)n) { perror(path); exit(2); }
    fclose(fp);
    *size = (size_t)n;
    return p;
}

int main(int argc, char **argv)
{
    int a;
    if (argc < 8 || (argc - 1) % 7) { fprintf(stderr, "usage: dict_finalize (SAMPLES SIZES CAP K D F OUT)...\n"); return 2; }
    for (a = 1; a < argc; a += 7) {
        size_t total = 0, textSize = 0, sum = 0, tail, contentSize, r;
        uint8_t *samples = slurp(argv[a], &total), *text = slurp(argv[a + 1], &textSize);
        size_t const cap = (size_t)strtoul(argv[a + 2], NULL, 10);
        unsigned const k = (unsigned)atoi(argv[a + 3]), d = (unsigned)atoi(argv[a + 4]), f = (unsigned)atoi(argv[a + 5]);
        unsigned n = 0, i;
        size_t *sizes, *exact;
        uint8_t *model = (uint8_t *)malloc(cap), *content, *dict = (uint8_t *)malloc(cap);
        uint32_t stats[448];
        uint64_t lits = 0, seqs = 0;
        char *txt = (char *)malloc(textSize + 1), *q;
        FILE *out;
        memcpy(txt, text, textSize); txt[textSize] = 0;
        sizes = (size_t *)malloc(sizeof(size_t) * (textSize / 2 + 2));
        for (q = txt; *q;) { char *e; unsigned long v = strtoul(q, &e, 10); if (e == q) break; sizes[n++] = v; sum += v; q = e; }
        if (sum != total || !n) { fprintf(stderr, "%s: sizes do not add up\n", argv[a + 1]); return 2; }
        exact = (size_t *)malloc(sizeof(size_t) * n);
        memcpy(exact, sizes, sizeof(size_t) * n);
        tail = model_train(samples, exact, n, model, cap, k, d, f);
        contentSize = cap - tail;
        content = (uint8_t *)malloc(contentSize ? contentSize : 1);
        memcpy(content, model + tail, contentSize);
        r = zso_trainStats(stats, content, contentSize, samples, exact, n, 3);
        if (zso_isError(r)) { fprintf(stderr, "zso_trainStats: %u\n", zso_errorCode(r)); return 1; }
        for (i = 0; i < 256; i++) lits += stats[i];
        for (i = 256; i < 320; i++) seqs += stats[i];
        r = zso_finalizeDictionary(dict, cap, content, contentSize, samples, exact, n, 3, 0);
        if (zso_isError(r)) { fprintf(stderr, "zso_finalizeDictionary: %u\n", zso_errorCode(r)); return 1; }
        printf("%zu %zu %llu %llu\n", contentSize, r, (unsigned long long)lits, (unsigned long long)seqs);
        out = fopen(argv[a + 6], "wb");
        if (!out || fwrite(dict, 1, r, out) != r) { perror(argv[a + 6]); return 2; }
        fclose(out);
        free(samples); free(text); free(txt); free(sizes); free(exact); free(model); free(content); free(dict);
    }
    return 0;
}
