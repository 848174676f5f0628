"""Sizes for the tests of k_emit2's group staging (tests/test_gpu_emit_staging.py and its child): widths that are multiples of four,
so the tile is staged in aligned groups of four pixels (chalkydri_amd/csrc/ck_emit_stage.h).  The frames are those of
tests/emit_row_cases.py.  Nothing here touches the GPU.

  68 x 18   a second tile column with one group inside the frame, a second tile row of two rows, the right halo column outside
  128 x 32  tiles whose right halo column and bottom halo row lie wholly outside the frame
  132 x 35  halo column and bottom halo row in another CCL tile (128 x 32) than the group rows; ragged in both directions
  196 x 34  a tile column whose groups span the CCL seam at x = 128 from the other side"""
SIZES = ((68, 18), (128, 32), (132, 35), (196, 34))
MIN_COMPONENT = (5, 25)
