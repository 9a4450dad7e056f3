// The ragged forms of the explicit-operator pair kernels, k_pairs_rag<NB, BAND> and k_pairs_cooph_rag<NB>, with their launch steps
// (the PairsRagArgs overloads of hgp_internal_pairs_all / _band / _listed): the text of hgp_pairs.hip compiled for a length per
// segment in a translation unit of its own.  The rectangular kernels of hgp_pairs.hip stay the code they were, and the two units build side by side.
#define HGP_PAIRS_RAGGED_TU 1
#define k_pairs k_pairs_rag
#define k_pairs_cooph k_pairs_cooph_rag
#include "hgp_pairs.hip"
