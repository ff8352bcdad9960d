// path_mapedit.hpp -- material edits in the photograph (matpbr_path.hip includes it; DESIGN.md section 1.4, "Material edits in the
// photograph"): the table of the path_kernel whose two walks differ in the material maps, not in the geometry, and the trait the
// kernel reads it by.
#pragma once
#include "path_reflect.hpp"

namespace {
// `Base` (NoObjects, or ShadeNormals with its map, which is not edited) and the edited maps beside the fitted ones of PathArgs.  A
// sample's first walk reads a_e, r_e, m_e at the vertices whose texel is masked and the fitted maps elsewhere; where it read a masked
// texel it is walked again on the fitted maps alone.  delta: the first walk's radiance minus the second's, over the samples walked
// twice; the radiance on the fitted maps of every sample (the second walk's, or the only one's) goes to PathArgs' `out`, which the
// entry point sets to `base`: the sum, the launch split and the final division are the render's own.
template <class Base>
struct MapEdit : Base {
    const float *a_e, *r_e, *m_e;   // [H,W,3], [H,W], [H,W]: the edited maps
    const uint8_t* mask;            // [H,W], non-zero = the edited maps are read there
    float* delta;                   // [H,W,3]
    uint32_t* rewalked;             // [H,W], nullable: second walks per pixel, added to
};
// what path_kernel reads off its table's type: the table carries edited maps and a sample takes up to two trips.  False for every
// other table.  (`EDIT` in the kernel is the transparency edit, TransEdit: another thing.)
template <class Objects> struct MapEditTraits { static constexpr bool mapedit = false; };
template <class Base> struct MapEditTraits<MapEdit<Base>> { static constexpr bool mapedit = true; };
}  // namespace
