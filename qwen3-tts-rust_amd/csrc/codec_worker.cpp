// codec_worker.cpp -- see codec_worker.h
#include "codec_worker.h"
#include <chrono>

namespace q3 {

CodecWorker::CodecWorker(CodecDecoder* codec, int dev, int n_lanes, int n_cs, size_t slot_cap) : codec_(codec), dev_(dev), st_(n_lanes), slot_cap_(slot_cap), n_cs_(n_cs) {
    for (auto& s : st_) Q3_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    Q3_HIP(hipHostMalloc((void**)&pcm_pinned_, (size_t)n_cs * slot_cap_ * sizeof(float)));
}

CodecWorker::~CodecWorker() {
    if (started_) {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; q_.hold = 0; }
        cv_.notify_all();
        thread_.join();
    }
    for (auto& c : comp_) (void)hipEventDestroy(c.ev);
    for (auto& kv : last_) (void)hipEventDestroy(kv.second.second);
    if (pcm_pinned_) (void)hipHostFree(pcm_pinned_);
    if (loud_pinned_.load()) (void)hipHostFree(loud_pinned_.load());
    for (auto s : st_) (void)hipStreamDestroy(s);
}

void CodecWorker::push(CodecJob* j, TaskKind kind, const int64_t* codes, int n_codes, bool is_final) {
    { std::lock_guard<std::mutex> lk(mu_); q_.push(j, kind, codes, n_codes, is_final); }
    cv_.notify_all();
}
void CodecWorker::purge(CodecJob* j) { std::lock_guard<std::mutex> lk(mu_); q_.purge(j); }
int CodecWorker::pending() { std::lock_guard<std::mutex> lk(mu_); return q_.pending; }

bool CodecWorker::poll_completion(bool block, Completion* out) {
    std::unique_lock<std::mutex> lk(mu_);
    if (!err_.empty()) throw Error("decoder thread: " + err_);
    if (comp_.empty()) {
        if (!block) return false;
        cv_.wait_for(lk, std::chrono::milliseconds(2));
        if (comp_.empty()) return false;
    }
    *out = comp_.front();
    if (!block && hipEventQuery(out->ev) != hipSuccess) return false;
    comp_.pop_front();
    q_.popped();
    lk.unlock();
    Q3_HIP(hipEventSynchronize(out->ev));
    return true;
}

unsigned char* CodecWorker::stage(const CodecJob& j, size_t add) const {
    const size_t at = j.pcm_enq * j.sample_bytes();
    Q3_CHECK(at + add <= slot_bytes(), "pcm staging overflow");
    return reinterpret_cast<unsigned char*>(pcm_pinned_ + (size_t)j.cs * slot_cap_) + at;
}

// [EXT] loudness: the thread's own; the allocation must not land inside another thread's stream capture
double* CodecWorker::loud_stage(const CodecJob& j, size_t add) {
    if (!loud_pinned_.load()) {
        std::lock_guard<std::mutex> cap(capture_mutex());
        double* p = nullptr;
        Q3_HIP(hipHostMalloc((void**)&p, (size_t)n_cs_ * loud_cap() * 2 * sizeof(double)));
        loud_pinned_.store(p);
    }
    Q3_CHECK(j.loud_enq + add <= loud_cap(), "loudness staging overflow");
    return loud_pinned_.load() + ((size_t)j.cs * loud_cap() + j.loud_enq) * 2;
}

// A job's tasks must run in order even when consecutive steps use different lanes.  A job's task alone stays on the job's lane.
int CodecWorker::pick_lane(const Step& s) {
    int lane = next_lane_;
    auto own = last_.find(s[0].job);
    if (s.size() == 1 && own != last_.end()) lane = own->second.first;
    else next_lane_ = (next_lane_ + 1) % (int)st_.size();
    for (const Task& t : s) {
        auto it = last_.find(t.job);
        if (it != last_.end() && it->second.first != lane) Q3_HIP(hipStreamWaitEvent(st_[lane], it->second.second, 0));
    }
    return lane;
}

void CodecWorker::start_stream(int lane, const Step& s) {
    CodecJob* j = s[0].job;
    if (j->pre_snap < 0) { codec_->reset_async(st_[lane], j->cs); return; } // AudioDecoder::create_state for a new request
    // [EXT] codec preambles: the stream starts from the snapshot; a converting one also from the preamble's tail
    codec_->restore_async(st_[lane], j->pre_snap, j->cs, pcm_format_native(j->out.fmt) ? nullptr : j->pre_tail);
    pre_restores++;
}

// engine.rs:520: decode the chunk(s), overlapping the next AR frames.  One pass serves the whole step: weights streamed once, one set of launches
void CodecWorker::decode_pass(int lane, const Step& s) {
    const int G = (int)s.size(), nf = (int)s[0].codes.size() / 16, spf = codec_->samples_per_frame();
    int n_low = 0;
    for (const Task& t : s) n_low += t.job->decode;
    dec_chunks += n_low;
    if (n_low < G) dec_shared += n_low;
    std::vector<int> streams(G); std::vector<float*> dst(G); std::vector<int64_t> codes((size_t)G * nf * 16);
    std::vector<OutSpec> out(G); std::vector<int64_t> n_out(G); // [EXT] what each stream is delivered as, what it was given
    std::vector<LoudDst> loud(G); std::vector<size_t> rows(G, 0); // [EXT] loudness: where each metered stream stands, the rows this chunk completes
    for (int g = 0; g < G; g++) {
        CodecJob* j = s[g].job;
        out[g] = j->out;
        // the samples that become available with these frames: of a stretched stream possibly none, at a slow rate more than native
        const size_t add = j->bytes_due((int64_t)nf * spf, false);
        if (j->out.loud) {
            rows[g] = (size_t)loud_blocks(j->tsm_native, (int64_t)nf * spf);
            loud[g].pos = j->tsm_native; loud[g].rows = loud_stage(*j, rows[g]);
        }
        j->tsm_native += (int64_t)nf * spf;
        streams[g] = j->cs; dst[g] = reinterpret_cast<float*>(stage(*j, add));
        std::copy(s[g].codes.begin(), s[g].codes.end(), codes.begin() + (size_t)g * nf * 16);
    }
    codec_->decode_group_async(st_[lane], G, streams.data(), codes.data(), nf, dst.data(), lane, out.data(), n_out.data(), loud.data());
    for (int g = 0; g < G; g++) { s[g].job->pcm_enq += (size_t)n_out[g]; s[g].job->loud_enq += rows[g]; }
}

// [EXT] speaking rate: the fence of a stretching request that was not cancelled flushes its stretcher -- the hops its last samples still owe --
// behind its last chunk (pick_lane has waited for it), before the fence's completion is recorded
void CodecWorker::flush_rate(int lane, const Step& s) {
    CodecJob* j = s[0].job;
    if (!j->stretched() || j->cancel.load() || j->cs < 0) return;
    const size_t add = j->bytes_due(0, true);
    int64_t n = 0;
    codec_->tsm_flush_async(st_[lane], j->cs, stage(*j, add), &n, lane);
    j->pcm_enq += (size_t)n;
}
// [EXT] codec preambles: a build's fence enqueues the snapshot behind its last chunk
void CodecWorker::snapshot_build(int lane, const Step& s) {
    CodecJob* j = s[0].job;
    if (j->snapshot && !j->cancel.load()) j->snap = codec_->snapshot_async(st_[lane], j->cs);
}

void CodecWorker::record(int lane, const Step& s) {
    for (const Task& t : s) {
        hipEvent_t ev = nullptr;
        if (t.kind != TASK_RESET) {
            Q3_HIP(hipEventCreate(&ev));
            Q3_HIP(hipEventRecord(ev, st_[lane])); // first one = the reference's first stream_tx.send (:522-523)
        }
        auto it = last_.find(t.job);
        if (t.kind == TASK_FENCE) { if (it != last_.end()) { (void)hipEventDestroy(it->second.second); last_.erase(it); } }
        else {
            hipEvent_t ord;
            if (it == last_.end()) { Q3_HIP(hipEventCreateWithFlags(&ord, hipEventDisableTiming)); last_[t.job] = {lane, ord}; }
            else { ord = it->second.second; it->second.first = lane; }
            Q3_HIP(hipEventRecord(ord, st_[lane]));
        }
        if (t.kind == TASK_RESET) continue;
        std::lock_guard<std::mutex> lk(mu_);
        comp_.push_back(Completion{t.job, ev, t.job->pcm_enq, t.kind == TASK_FENCE, t.job->loud_enq});
        if (t.kind == TASK_CHUNK) codec_calls_++;
    }
    cv_.notify_all();
}

void CodecWorker::main() {
    try {
        Q3_HIP(hipSetDevice(dev_)); // HIP's current device is per thread
        const int gmax = codec_->max_group();
        for (;;) {
            Step s;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || q_.ready(); });
                s = q_.take(gmax);
                if (s.empty()) return;
            }
            const int lane = pick_lane(s);
            if (s[0].kind == TASK_RESET) start_stream(lane, s);
            else if (s[0].kind == TASK_CHUNK) decode_pass(lane, s);
            else { flush_rate(lane, s); snapshot_build(lane, s); }
            record(lane, s);
        }
    } catch (const std::exception& ex) {
        std::lock_guard<std::mutex> lk(mu_);
        err_ = ex.what();
        cv_.notify_all();
    }
}

} // namespace q3
