// kept_rows.hpp -- KeptRows: what a pass with one lane per on-screen row of a kept frame reads -- the preprocess-backward in
// its three forms, the camera gradient, the densify statistics, the depth-to-position pass, the contrib zero and fold, the
// slice bounds, the touched-row marking.  The per-row counterpart of KeptFrame (kept_walk.hpp), host side only: a launcher
// takes it plus what is its own and unpacks it at the launch, so the kernels keep their signatures.  Built by
// abi_internal.hpp (kept_rows: the context's last keep-state frame; owner_slot_rows: a view of an ownership step).
#pragma once

#include "launch.hpp"

namespace lcgs
{
struct KeptRows {
    CamParams cp;
    float     scale_modifier;
    int       sh_deg;
    const float *pos, *scale, *rotq, *sh, *opacity; // the scene's rows (opacity: read only for a row of an antialiased frame)
    const uint32_t*    vis_index; // on-screen row -> scene row, ascending
    const uint32_t*    d_counts;  // [0] = on-screen rows
    const float*       grads2d;   // kG2D floats per on-screen row
    const float4*      shjac;     // the kept colour Jacobian, 3 x float4 per on-screen row; NULL: the frame kept none
    const SplatRecord* recs;      // (NULL for an ownership slot: its passes read none)
    int64_t            P;         // rows of the scene arrays
    int64_t            hint;      // the launch size in rows (larger live counts are strided)
};
} // namespace lcgs
