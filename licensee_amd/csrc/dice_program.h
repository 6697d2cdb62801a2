// Template-specialized sparse scoring program: setup and launches (dice_program.cpp). The program
// itself, its plan and its source, is dice_program_gen.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/licensee_dice.h"
#include "dice_program_gen.h"

namespace dice {

int program_setup(dice_ctx* c, const dice_templates* t);
// compact tile: b->d_rows[0, n) -> b->d_tiles
int program_launch_pack(dice_ctx* c, dice_batch* b, int64_t n, hipStream_t s);
int program_launch_match(dice_ctx* c, dice_batch* b, double thr, hipStream_t s);
int program_launch_matrix(dice_ctx* c, dice_batch* b, int32_t k, hipStream_t s);
// the ranking alone, into b->d_tki / b->d_tks ([k][n]); k >= 1
int program_launch_topk(dice_ctx* c, dice_batch* b, int32_t k, hipStream_t s);

}  // namespace dice
