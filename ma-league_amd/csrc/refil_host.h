// refil_host.h -- host-side pieces the REFIL translation units (refil.hip, refil_layers.hip, refil_grad.hip) share.
#pragma once
#include "../../include/maleague.h"

// entity input width: the entity features, plus the one-hot last action when the dims ask for it
inline int refil_d0(const MlgRefilDims* d) { return d->entity_shape + (d->entity_last_action ? d->n_actions : 0); }

int check_refil_dims(const MlgRefilDims* d);        // agent ops and rollout (refil.hip)
int check_refil_mixer_dims(const MlgRefilDims* d);  // FlexQMixer ops (refil_layers.hip)
