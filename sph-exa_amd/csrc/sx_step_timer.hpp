/*! @file sx_step_timer.hpp
 * @brief stage and kernel times of one sx_sim step, by name: what sx_sim_stage_times / sx_sim_kernel_times report
 *        (and, at the end, StageClock: the stage times of one call of an analysis)
 *
 * A step calls start(), marks "stage X ends here" and "kernel X begins / ends" on its stream where they happen, and
 * calls collect() once the stream is synchronised.  A stage runs from the last boundary recorded before its end mark
 * (the start of the step or another stage's end) to that mark; a stage or kernel a step does not mark reads 0.0.  Every
 * propagator reports the same names in the same order (consumers index by position) and marks the ones it has.
 */
#pragma once

#include <hip/hip_runtime.h>

namespace sx::sim
{

// the stages of a step and the hot kernels timed on their own, in reported order; the enumerators are spelled as the
// reported names.  nbodyIntegrate is reported by propagator 3 only
// clang-format off
enum class Stage : int { sync, FindNeighbors, XMass, VeDefGradh, EOS, IadDivvCurlv, AVswitches, MomentumEnergy, Gravity,
                         UpdateQuantities, count };
enum class Kernel : int { findNeighbors, xmass, veDefGradh, iadDivvCurlv, avSwitches, momentumEnergy, gravity,
                          nbodyIntegrate, count };
// clang-format on
constexpr int kNumStages = (int)Stage::count, kNumKernels = (int)Kernel::count;

inline constexpr const char* kStageNames[kNumStages]   = {"sync",         "FindNeighbors", "XMass",          "VeDefGradh",
                                                          "EOS",          "IadDivvCurlv",  "AVswitches",     "MomentumEnergy",
                                                          "Gravity",      "UpdateQuantities"};
inline constexpr const char* kKernelNames[kNumKernels] = {"findNeighbors", "xmass",          "veDefGradh", "iadDivvCurlv",
                                                          "avSwitches",    "momentumEnergy", "gravity",    "nbodyIntegrate"};
// the kernels of the radiative cooling (sx_cool.hpp), marked by a sim that cools: slots of their own, read through
// sx_sim_cooling_times, so that the names and positions above stay what consumers index by
enum class Cooling : int { coolingTime, cool, count };
constexpr int kNumCooling = (int)Cooling::count;

class StepTimer
{
public:
    float stageMs[kNumStages]{}, kernelMs[kNumKernels]{}, coolingMs[kNumCooling]{};

    StepTimer() { forEachEvent([](hipEvent_t& e) { (void)hipEventCreate(&e); }); }
    ~StepTimer() { forEachEvent([](hipEvent_t& e) { if (e) (void)hipEventDestroy(e); }); }
    StepTimer(const StepTimer&)            = delete;
    StepTimer& operator=(const StepTimer&) = delete;

    //! the start of a step: nothing is marked yet
    hipError_t start(hipStream_t st)
    {
        for (auto& f : stageFrom_)
            f = nullptr;
        for (auto& k : kernelState_)
            k = kIdle;
        for (auto& k : coolingState_)
            k = kIdle;
        last_ = start_;
        return hipEventRecord(start_, st);
    }

    //! stage g ends here; it began at the last boundary recorded before
    hipError_t stageEnd(Stage g, hipStream_t st)
    {
        stageFrom_[(int)g] = last_;
        last_              = stageEnd_[(int)g];
        return hipEventRecord(last_, st);
    }

    //! kernel k begins (again: a repeated attempt drops the interval of the earlier one)
    hipError_t begin(Kernel k, hipStream_t st)
    {
        kernelState_[(int)k] = kBegun;
        return hipEventRecord(kernel_[(int)k][0], st);
    }

    hipError_t end(Kernel k, hipStream_t st)
    {
        kernelState_[(int)k] = kernelState_[(int)k] == kBegun ? kDone : kIdle;
        return hipEventRecord(kernel_[(int)k][1], st);
    }

    hipError_t coolingBegin(Cooling k, hipStream_t st)
    {
        coolingState_[(int)k] = kBegun;
        return hipEventRecord(cooling_[(int)k][0], st);
    }

    hipError_t coolingEnd(Cooling k, hipStream_t st)
    {
        coolingState_[(int)k] = coolingState_[(int)k] == kBegun ? kDone : kIdle;
        return hipEventRecord(cooling_[(int)k][1], st);
    }

    //! after the stream's synchronisation: the times of what this step marked, 0.0 for the rest
    void collect()
    {
        for (int g = 0; g < kNumStages; ++g)
            stageMs[g] = stageFrom_[g] ? elapsed(stageFrom_[g], stageEnd_[g]) : 0.f;
        for (int k = 0; k < kNumKernels; ++k)
            kernelMs[k] = kernelState_[k] == kDone ? elapsed(kernel_[k][0], kernel_[k][1]) : 0.f;
        for (int k = 0; k < kNumCooling; ++k)
            coolingMs[k] = coolingState_[k] == kDone ? elapsed(cooling_[k][0], cooling_[k][1]) : 0.f;
    }

private:
    enum : unsigned char { kIdle, kBegun, kDone };

    static float elapsed(hipEvent_t a, hipEvent_t b)
    {
        float ms = 0.f;
        return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f;
    }

    template<class F>
    void forEachEvent(F&& fn)
    {
        fn(start_);
        for (auto& e : stageEnd_)
            fn(e);
        for (auto& pair : kernel_)
            fn(pair[0]), fn(pair[1]);
        for (auto& pair : cooling_)
            fn(pair[0]), fn(pair[1]);
    }

    hipEvent_t    start_{nullptr}, stageEnd_[kNumStages]{}, kernel_[kNumKernels][2]{}, cooling_[kNumCooling][2]{};
    hipEvent_t    last_{nullptr};           // the last boundary recorded in this step
    hipEvent_t    stageFrom_[kNumStages]{}; // where each stage marked in this step began; nullptr: not marked
    unsigned char kernelState_[kNumKernels]{}, coolingState_[kNumCooling]{};
};

} // namespace sx::sim

namespace sx
{

/*! the times of the N consecutive stages of one call of an analysis (sx_fof.hip, sx_twopoint.hip, sx_profile.hip)
 *  between N + 1 boundaries on its stream.  A call begins the clock, marks its boundaries where they happen and
 *  finishes it once the stream is synchronised; with the clock off nothing is recorded and the figures are zeros */
template<int N>
struct StageClock
{
    bool       on{false};
    float      ms[N]{}; //!< of the last call
    hipEvent_t ev[N + 1]{};

    //! the start of a call: no figure yet; the events are created by the first call that is timed
    hipError_t begin()
    {
        for (float& m : ms)
            m = 0.f;
        if (on)
            for (auto& e : ev)
                if (!e)
                    if (hipError_t rc = hipEventCreate(&e); rc != hipSuccess) return rc;
        return hipSuccess;
    }

    //! boundary k lies here: stage k - 1 ends and stage k begins (marked again: it lies here instead)
    hipError_t mark(int k, hipStream_t s) { return on ? hipEventRecord(ev[k], s) : hipSuccess; }

    //! after the stream's synchronisation, all boundaries marked: the times, 0 where one cannot be read
    void finish()
    {
        if (on)
            for (int k = 0; k < N; ++k)
                if (hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]) != hipSuccess) ms[k] = 0;
    }

    void release()
    {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e), e = nullptr;
    }
};

} // namespace sx
