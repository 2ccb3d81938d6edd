// The learners' values of a sweep as the kernels take them (evac_sweep.h: the linear learners' kernels; evac_encoder_sweep.h: the
// encoder leaders'), apart from the kernels so that the units which only fill or forward them define none of evac_sweep.h's
// plain __global__s a second time.  Arrays by value, read at the learner's index; the lone trainer's number types.
#pragma once

#include <cstdint>

#include "evac_learner.h"

namespace evac {

struct LearnerLoss {                            // RpoArgs.clip / ent / vf / alpha per learner: 1 KiB
    float clip[kMaxLearners], ent[kMaxLearners], vf[kMaxLearners], alpha[kMaxLearners];
};
struct LearnerSteps {                           // AdamArgs.lr / target_kl / max_norm / use_target_kl per learner: 1.3 KiB
    double lr[kMaxLearners], target_kl[kMaxLearners];
    float max_norm[kMaxLearners];
    uint64_t use_target_kl;                     // bit s: learner s has a target
};
struct LearnerDiscounts {                       // k_gae's gamma and gl per learner: 512 bytes
    float gamma[kMaxLearners], gl[kMaxLearners];
};

}  // namespace evac
