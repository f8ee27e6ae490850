# Round check, then keep only the summaries that go to profiles/ (small enough to copy off the GPU box)
set -o pipefail
R=${R:-r3}
export O=${O:-round_out}
mkdir -p $O
R=$R bash tools/gpu_round_check.sh > $O/round_check.log 2>&1
rc=$?
# the learner's SQ counters and learn() time at P = 8 / 4 / 2 / 1
if [ $rc -eq 0 ]; then
  bash tools/learner_pmc_r3.sh > $O/learner_pmc_run.log 2>&1 && bash tools/learn_time_sweep.sh >> $O/learner_pmc_run.log 2>&1
  rc=$?
fi
mkdir -p ${O}_keep
cp $O/learner_pmc.txt ${O}_keep/${R}_learner_pmc.txt 2>/dev/null
cp $O/learn_sweep.log ${O}_keep/${R}_learn_sweep.log 2>/dev/null
cp $O/learner_pmc_run.log ${O}_keep/ 2>/dev/null
cp $O/round_check.log $O/pytest_gpu.log $O/bench_full.json $O/bench_full.err ${O}_keep/ 2>/dev/null
cp $O/${R}_*.json ${O}_keep/ 2>/dev/null
find $O/prof_$R -name "*kernel_stats.csv" -exec cp {} ${O}_keep/${R}_kernel_stats.csv \; 2>/dev/null
find $O/prof_c3_$R -name "*kernel_stats.csv" -exec cp {} ${O}_keep/${R}_config3_kernel_stats.csv \; 2>/dev/null
rm -rf $O/*
mv ${O}_keep $O/keep
echo rc=$rc
exit $rc
