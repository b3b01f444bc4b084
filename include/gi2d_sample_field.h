/* One field of a batched sampling call (gi2d.h "batched samples"; DESIGN.md 3.8 "Batched samples"): what the single
 * sampling entries of gi2d.h take per field, by name and with the same meaning.  gi2d.h includes this header, so a caller
 * includes gi2d.h alone; the Python binding derives the ctypes form from this text as it derives every other structure
 * (gaussianimage_plus_amd/_lib.py).  The structure is also the layout of one entry of the device table
 * gi2d_sample_batch_table writes. */
#ifndef GI2D_SAMPLE_FIELD_H
#define GI2D_SAMPLE_FIELD_H

#include <stdint.h>

typedef struct gi2d_sample_field {
    int num_points, capacity, tiles_x, tiles_y;
    unsigned img_width, img_height;
    const int32_t *gaussian_ids_sorted, *tile_bins;
    int tile_bins_rows;
    float max_filter; /* 0: a plain field (covs NULL) */
    const float *xys, *conics, *covs, *colors, *opacities;
    const int32_t *status;
} gi2d_sample_field;

#endif /* GI2D_SAMPLE_FIELD_H */
