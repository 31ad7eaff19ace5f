/*  fast5_dac.h -- a read as a multi-read fast5 file holds it: 16-bit DAC values and the read's calibration, pA = (dac + offset) * raw_unit with
 *  raw_unit = range / digitisation in float.  Shared by the cursor (fast5_interface.h) and the libhdf5-free walker (flappie_amd/host/fast5_raw.h). */
#ifndef FFHIP_FAST5_DAC_H
#define FFHIP_FAST5_DAC_H
#include <stddef.h>
#include <stdint.h>
typedef struct { char *uuid; int16_t *dac; size_t n; float offset, raw_unit; } fast5_dac_read;
#endif
