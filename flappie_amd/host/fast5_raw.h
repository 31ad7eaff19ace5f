/*  fast5_raw.h -- fast5 files read without libhdf5 (fast5_raw.c): the fast path of read_raw and of the multi-read cursor (fast5_interface.c).
 *  Replaces, for the files it knows, the libhdf5 calls of /root/reference/src/fast5_interface.c:231-318. */
#ifndef FFHIP_FAST5_RAW_H
#define FFHIP_FAST5_RAW_H
#include <stddef.h>
#include <stdint.h>
#include "../../include/fast5_dac.h"

typedef struct { char *uuid; float *raw; size_t n; } fast5_raw_read;

/* 1: `out` holds malloc'd `uuid` (the read_id attribute) and `raw` (n samples, scaled to pA if asked) -- the values read_raw's
 * libhdf5 path gives; 0: a file (or a part of it) this reader does not know: nothing allocated, ask libhdf5. */
int fast5_read_raw_fast(const char *filename, int scale_to_pA, fast5_raw_read *out);


/* A multi-read file, mapped: its read_<x> groups in strcmp order of their names.
 * fast5_walk_open: 1 = a multi-read file, *w set; 0 = not one (a `Raw` child in the root group, or no read_<x>); -1 = a file or a root group this reader
 * does not know (dense link storage, ...): ask libhdf5.  fast5_walk_read: 1 = `out` holds malloc'd uuid and dac; 0 = this read is left to libhdf5. */
typedef struct fast5_walk fast5_walk;
int fast5_walk_open(const char *filename, fast5_walk **w);
size_t fast5_walk_count(const fast5_walk *w);
const char *fast5_walk_name(const fast5_walk *w, size_t i);
int fast5_walk_read(const fast5_walk *w, size_t i, fast5_dac_read *out);
void fast5_walk_close(fast5_walk *w);
#endif
