// out_chain.h -- [EXT] what happens to a chunk behind the codec's output conv (q3tts_spec.h "output formats", "speaking rate", "pitch",
// "volume", "loudness"), as one object beside the decoder: the five stages (out_stages.h), each made by the first call that needs it, their
// per-lane buffers and argument arrays, what every stream was last stretched or shifted with, and the counters.  Which stage runs, what it is
// handed and where every stream's copy comes from is out_route's arithmetic (sched_logic.h); the chain launches through the stages'
// launchers alone.  One owner thread -- the one that issues the decodes; stats() may be called from any.
#pragma once
#include "out_stages.h"
#include <memory>

namespace q3 {

class OutChain {
public:
    // lane_floats = floats of a lane's native chunk buffer, gmax streams' worth: what sizes every stage's lane buffers
    OutChain(int n_streams, int gmax, int n_lanes, size_t lane_floats);
    // Behind the output conv on `st`: native = the pass's chunk [G][T] on lane `lane`, stream g of slot streams[g] delivered as out[g] (NULL:
    // every stream plain).  One meter launch over the metered streams, whose rows go to loud[g].rows; one volume launch, in place; one launch
    // of each stage a stream of the pass belongs to; then every stream's copy to dst[g] (pinned) of the n_out[g] (optional) samples its stage
    // made.  A pass of native streams is G copies
    void run(hipStream_t st, int lane, int G, int T, const int32_t* streams, float* native, const OutSpec* out, const LoudDst* loud, float* const* dst,
             int64_t* n_out);
    // the end of a stretched or shifted utterance: one launch without input, then the copy of the *n_out samples it completes to dst (pinned).
    // A stream that was neither since its reset gives nothing
    void flush(hipStream_t st, int lane, int s, void* dst, int64_t* n_out);
    void reset(hipStream_t st, int s);                            // stream s starts from zeros in every stage that exists
    void restore(hipStream_t st, int s, const float* pcm_tail);   // a primed stream: as reset, but the converter's history is left alone or, with pcm_tail (Q3_PCM_HIST pinned floats), starts as those samples
    OutputStageStats stats() const { return count_.snapshot(); }
private:
    // a stage and lane[l] = what it makes of a pass on lane l (none for a stage that works in place)
    template <class Stage, class T = float> struct Lazy { using stage_type = Stage; std::unique_ptr<Stage> stage; std::vector<DevBuf<T>> lane; };
    template <class L> typename L::stage_type& ensure(L& l, size_t lane_elems);
    void reset_prosody(hipStream_t st, int s);
    size_t region() const { return 2 * (lane_floats_ / (size_t)gmax_) + 8 * Q3_TSM_HOP; }   // floats per stream of the stretcher's and the shifter's lane buffers: a chunk of T samples gives at most 2 T samples plus a hop at rate 50 and 2 T + 961 at the tempo 1/2, a flush at most six hops or 3361 samples
    size_t loud_rows() const { return lane_floats_ / (size_t)gmax_ / Q3_LOUD_BLOCK + 1; }   // rows per stream of the meter's
    int n_streams_, gmax_, n_lanes_; size_t lane_floats_;
    StageCounters count_;
    Lazy<PcmConverter> conv_; Lazy<TsmStretcher> tsm_; Lazy<PitchShifter> pitch_; Lazy<VolumeStage> vol_; Lazy<LoudnessStage, double> loud_;
    // per lane, for the pass in flight: the route, the meter's positions, and what the launchers report -- the converter's counts, the
    // stretcher's and the shifter's (shared), the meter's rows
    struct Lane { OutRoute route; std::vector<int64_t> lpos, cnt, scnt, lcnt; };
    std::vector<Lane> lanes_;
    // prosody_[s] = what stream s was last stretched or shifted with since its reset, which is what its flush runs with; live = false:
    // neither since the reset, or flushed
    struct Prosody { OutSpec out; bool live = false; };
    std::vector<Prosody> prosody_;
};

} // namespace q3
