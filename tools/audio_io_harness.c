// audio_io_harness.c - the upload decoder (csrc/audio_io.c) over files from the command line, as a stand-alone CPU program: meant to
// be built plain and with AddressSanitizer / UBSan (command lines in tools/README.md) and run over the corpus that
// `python tests/audio_corpus.py OUTDIR` writes.  Never loaded into Python, never run on a GPU machine.
//
// Linked with -Wl,--wrap=malloc,--wrap=realloc, it sees every allocation the decoder asks for: a single request above 128 MiB is a
// failure (and is answered with NULL, so that the run goes on without touching the memory).  128 MiB is a condition, not a measurement:
// a corpus file is under 1 MB and decodes to fewer than 2^21 samples, 8 MiB of PCM beside the 4 MiB subframe buffer.
//
// Exit status 0: every file returned WIS_OK or WIS_E_FORMAT / WIS_E_CHECKSUM / WIS_E_NOMEM, an error left no buffer behind, no request
// was above the limit (and no sanitizer stopped the run).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "wis_hip.h"

#define LIMIT ((size_t)128 << 20)

void* __real_malloc(size_t n);
void* __real_realloc(void* p, size_t n);
static int in_decode = 0;
static size_t largest = 0, over_limit = 0;

static int note(size_t n) {
  if (!in_decode) return 0;
  if (n > largest) largest = n;
  if (n > LIMIT) { ++over_limit; return 1; }
  return 0;
}
void* __wrap_malloc(size_t n) { return note(n) ? NULL : __real_malloc(n); }
void* __wrap_realloc(void* p, size_t n) { return note(n) ? NULL : __real_realloc(p, n); }

int main(int argc, char** argv) {
  long n_ok = 0, n_refused = 0, n_bad = 0, n_files = 0;
  size_t largest_before = 0;
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) { fprintf(stderr, "%s: cannot open\n", argv[a]); return 2; }
    fseek(f, 0, SEEK_END);
    long len = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* buf = (uint8_t*)malloc(len > 0 ? (size_t)len : 1);  // exactly as long as the file: a read past its end is the sanitizer's to see
    if (!buf || (len > 0 && fread(buf, 1, (size_t)len, f) != (size_t)len)) { fprintf(stderr, "%s: cannot read\n", argv[a]); return 2; }
    fclose(f);
    ++n_files;
    float* pcm = NULL; int64_t n = -1; int sr = -1, md5 = -7;
    in_decode = 1;
    int rc = wis_audio_decode(len > 0 ? buf : (uint8_t*)"", (size_t)len, &pcm, &n, &sr, &md5);
    in_decode = 0;
    if (largest > largest_before) {
      if (largest > LIMIT) fprintf(stderr, "%s: asked for %zu bytes\n", argv[a], largest);
      largest_before = largest;
    }
    if (rc == WIS_OK) {
      if (!pcm || n < 0 || sr <= 0) { fprintf(stderr, "%s: WIS_OK with pcm %p, %lld samples, %d Hz\n", argv[a], (void*)pcm, (long long)n, sr); ++n_bad; }
      else {
        volatile float sum = 0.f;  // touch every sample: the buffer is as long as the decoder says
        for (int64_t i = 0; i < n; ++i) sum += pcm[i];
        ++n_ok;
      }
      wis_audio_free(pcm);
    } else if (rc == WIS_E_FORMAT || rc == WIS_E_CHECKSUM || rc == WIS_E_NOMEM) {
      if (pcm) { fprintf(stderr, "%s: error %d left a buffer behind\n", argv[a], rc); ++n_bad; }
      ++n_refused;
    } else {
      fprintf(stderr, "%s: return code %d\n", argv[a], rc); ++n_bad;
    }
    free(buf);
  }
  printf("%ld files: %ld decoded, %ld refused, %ld wrong; largest single request %zu bytes; %zu requests above %zu\n",
         n_files, n_ok, n_refused, n_bad, largest, over_limit, LIMIT);
  return (n_bad || over_limit) ? 1 : 0;
}
