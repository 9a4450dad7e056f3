// The ragged form of the solve-based pair kernel, k_pairs_acc_rag<NB>, with its launch step (hgp_internal_pairs_acc, std::true_type): the
// text of hgp_pairs_acc.hip compiled for AccRagArgs - a length per segment - in a translation unit of its own (see hgp_pairs_ragged.hip).
#define HGP_PAIRS_RAGGED_TU 1
#define k_pairs_acc k_pairs_acc_rag
#include "hgp_pairs_acc.hip"
