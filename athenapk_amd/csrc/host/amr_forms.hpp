// amr_forms.hpp -- the forms of the multilevel ghost exchange, stated once.
//
// A form is a FAMILY -- which decides the message set, the pack and unpack lists, the prolongation operators, the
// block-boundary lists and the half after the messages -- plus its own same-rank fill list and the half in front of
// the messages.  restrict_own (first in the front half) and coarse_bc (between unpack and prolongation) belong to all.
//
//   form          family  fills
//   FULL          full    every ghost zone
//   FACES         faces   those straight behind block faces: not the ones behind edges and corners, which no sweep or
//                         flux correction reads
//   DIRECT        faces   ... nor those behind faces shared with a same-rank block of the same level, which the stages
//                         read from that block's interior through the face table (amr_direct)
//   SHELL         shell   every ghost zone, edges and corners too, AMR_SHELL_DEPTH layers deep: what the tagging
//                         criteria and a donor-cell / PLM first stage read
//   SHELL_DIRECT  shell   ... without the zones behind same-rank same-level faces: the tag kernel, ConsToPrim and the
//                         next predictor follow the face table there
#pragma once

namespace apk {

enum { AMR_XCHG_FULL = 0, AMR_XCHG_FACES, AMR_XCHG_DIRECT, AMR_XCHG_SHELL, AMR_XCHG_SHELL_DIRECT, AMR_XCHG_FORMS };
enum { AMR_FAMILY_FULL = 0, AMR_FAMILY_FACES, AMR_FAMILY_SHELL, AMR_FAMILIES };

constexpr int AMR_SHELL_DEPTH = 2;  // ghost layers of the shell exchange (refinement/gradient.cpp:33-36 reads [s-2, e+2]^3)

struct AmrFamilyInfo {
  const char *tag;  // allocator tag of the family's message buffers
  int bc;           // the family whose block-boundary lists run after its prolongation (its own, or borrowed)
  int whole;        // the form whose same-rank fill list leaves none of the family's zones out
};
constexpr AmrFamilyInfo AMR_FAMILY[AMR_FAMILIES] = {
    {"halo", AMR_FAMILY_FULL, AMR_XCHG_FULL},
    {"halo_faces", AMR_FAMILY_FULL, AMR_XCHG_FACES},  // (borrows the full family's block boundaries)
    {"halo_shell", AMR_FAMILY_SHELL, AMR_XCHG_SHELL},
};
constexpr int AMR_FORM_FAMILY[AMR_XCHG_FORMS] = {AMR_FAMILY_FULL, AMR_FAMILY_FACES, AMR_FAMILY_FACES, AMR_FAMILY_SHELL,
                                                 AMR_FAMILY_SHELL};

}  // namespace apk
