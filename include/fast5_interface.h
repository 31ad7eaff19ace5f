/*  fast5_interface.h -- fast5 input (single-read files as the reference reads them; multi-read files through a cursor) and `--trace` HDF5 output.
 *  Same signatures as /root/reference/src/fast5_interface.h:17-23.  Built only when libhdf5 is available
 *  (FLAPPIE_HAVE_HDF5); the HIP engine does not depend on it.
 */
#ifndef FFHIP_FAST5_INTERFACE_H
#define FFHIP_FAST5_INTERFACE_H
#include <hdf5.h>
#include <stdbool.h>
#include <stdint.h>
#include "fast5_dac.h"
#include "flappie_structures.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fast5_interface.c:231-318: /Raw/Reads/<first entry>/Signal + its `read_id`, optionally scaled to pA with
 * /UniqueGlobalKey/channel_id {digitisation, offset, range}.  raw == NULL on failure. */
raw_table read_raw(const char *filename, bool scale_to_pA);
/* the same through libhdf5 only: read_raw tries host/fast5_raw.c first (a single-read file walked in memory, no libhdf5 call) and comes here for every file
 * that reader does not know (not in the reference's header) */
raw_table read_raw_hdf5(const char *filename, bool scale_to_pA);
/* ---- multi-read files (not in the reference, which reads single-read files only): one file, thousands of reads, each a root group
 * read_<x> { Raw { Signal (int16), read_id }, channel_id { digitisation, offset, range } }.  A file is multi-read when its root group has no `Raw` child and at
 * least one child whose name begins with "read_"; the root attribute `file_type` is not required.
 * A read comes as the file holds it -- DAC values and calibration, pA = (dac + offset) * raw_unit with raw_unit = range / digitisation in float, the
 * expressions of read_raw -- so that the scaling can be done where the samples are used (ffhip_prep_create_dac).  uuid: the `read_id` attribute of Raw,
 * or <x> where a file has none.  Reads come in increasing strcmp order of their group names (H5Literate's H5_INDEX_NAME / H5_ITER_INC): the order is a
 * property of the file.  As for single-read files, host/fast5_raw.c walks the files it knows without libhdf5 (the file mapped, not copied) and libhdf5
 * reads whatever that walker refuses -- a whole file or a single read -- with the same values in the same order.  A Signal behind a filter libhdf5
 * has no plugin for (VBZ, filter 32020, is found through HDF5_PLUGIN_PATH) is reported by the filter's number and the cursor goes on. */
typedef struct fast5_multi fast5_multi;
/* NULL: not a multi-read file (or not a readable file at all: read_raw says which) */
fast5_multi *fast5_multi_open(const char *filename);
/* 1: `out` holds the next read (uuid and dac are malloc'd: the caller frees them); 0: no read is left; -1: the next read could not be read -- it was
 * reported (warnx) and skipped, the call after this one gives the read behind it */
int fast5_multi_next(fast5_multi *m, fast5_dac_read *out);
void fast5_multi_close(fast5_multi *m);
/* the same cursor held to one of its two paths (tests, FLAPPIE_DEBUG=hdf5_read): 1 = host/fast5_raw.c's walker only (NULL where it refuses the file; a read
 * it refuses is a -1), 2 = libhdf5 only */
fast5_multi *fast5_multi_open_path(const char *filename, int path);
/* reads of the file, and the group name of the read the next call of fast5_multi_next gives (NULL behind the last) */
size_t fast5_multi_count(const fast5_multi *m);
const char *fast5_multi_next_name(const fast5_multi *m);

/* one call per file for a reader that takes both kinds: a single-read file's table (read_raw's, *multi == NULL) or the cursor over a multi-read file */
raw_table read_raw_or_multi(const char *filename, bool scale_to_pA, fast5_multi **multi);

/* fast5_interface.c:59-74: -1 if filename is NULL; opens an existing file read-write, else creates it */
hid_t open_or_create_hdf5(const char *filename);
/* fast5_interface.c:321-349: group `readname` with `signal` (f32, trimmed normalised signal) and `trace`
 * (u8 [nblock+1 x nstate]), shuffle + deflate when compression_level > 0 */
void write_summary(hid_t hdf5file, const char *readname, const struct _raw_basecall_info res, hsize_t chunk_size,
                   int compression_level);

/* The same group in two steps, for writers that want the compression off the HDF5 lock: summary_pack_create does the
 * filters' work (shuffle + deflate per chunk, the u8 conversion of the trace) WITHOUT calling libhdf5 -- any number of threads may
 * run it --, summary_pack_write creates the datasets with the properties write_summary uses and hands the finished chunks over
 * (H5Dwrite_chunk).  A file written this way reads back exactly like one written by write_summary. */
typedef struct summary_pack summary_pack;
summary_pack *summary_pack_create(const struct _raw_basecall_info res, hsize_t chunk_size, int compression_level);
void summary_pack_write(hid_t hdf5file, const char *readname, const summary_pack *pack);
void summary_pack_free(summary_pack *pack);

#ifdef __cplusplus
}
#endif
#endif
