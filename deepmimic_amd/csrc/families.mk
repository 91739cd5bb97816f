# Included by deepmimic_amd/csrc/Makefile and tests/emu/Makefile (after OBJDIR): the kernel objects, one per precision and family id of dm_families.h --
# the id of every F( row of DM_STEP_FAMILIES and DM_MISC_FAMILY.  Neither Makefile restates the list.  (${shell }: the pattern's parentheses are unbalanced.)
FAMILIES_H := $(dir $(lastword $(MAKEFILE_LIST)))dm_families.h
KIDS := ${shell sed -n -e 's/^ *F(\([0-9][0-9]*\),.*/\1/p' -e 's/^.define DM_MISC_FAMILY \([0-9][0-9]*\).*/\1/p' $(FAMILIES_H)}
ifeq ($(strip $(KIDS)),)
$(error no family ids found in $(FAMILIES_H))
endif
KOBJS := $(foreach i,$(KIDS),$(OBJDIR)/k_f32_$(i).o $(OBJDIR)/k_f64_$(i).o)
# HOST_HDRS: the headers dm_host.cpp includes besides HDRS, relative to this directory; both dm_host.o rules depend on every one (tests/test_build_rules.py)
HOST_HDRS := dm_policy.h dm_policy_host.h dm_scene_load.h dm_norm.h dm_returns.h dm_ppo_batch.h dm_replay.h dm_episode.h dm_amp_rewards.h dm_math_probe.h dm_time_warp.h dm_link_state.h dm_kin_query.h dm_state_pool.h dm_push.h dm_train.h dm_train_gated.h dm_optim.h
