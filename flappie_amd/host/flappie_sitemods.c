/*  flappie_sitemods.c -- the lines of flappie --remap-mods (include/flappie_sitemods.h) */
#include "../../include/flappie_sitemods.h"

int flappie_sitemods_write(FILE *out, const char *name, const uint8_t *codes, size_t L, const char *alphabet, const ffhip_site_mod *sm, size_t nsm) {
    for (size_t k = 0; k < nsm; k++) {
        if (sm[k].pos < 0 || (size_t)sm[k].pos >= L) return -1;
        const char letter = alphabet[codes[sm[k].pos]];
        if ('C' != letter && 'Z' != letter) return -1;
        fprintf(out, "%s\t%d\t%c\t%d\t%.9g\t%.9g\t%.9g\n", name, (int)sm[k].pos, letter, (int)sm[k].nblock, (double)sm[k].can, (double)sm[k].mod,
                (double)sm[k].can - (double)sm[k].mod);
    }
    return 0;
}
