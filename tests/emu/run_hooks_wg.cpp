// TEST INFRASTRUCTURE -- the workgroup form of the SQP (nlmpc_sqp_wg, include/mpcx/nlmpc_sqp_wg.hpp) instantiated for whole-vector hooks
// (mpcx::HookModel of include/mpcx/nlmpc_hooks.hpp) and stepped through on the host by the lock-step interpreter of tests/emu/hip/hip_runtime.h:
// no GPU, nothing of libmpcx.so.  The three systems of tests/test_nlmpc_hooks.py written as functors with the reference's hook signatures
// (IDimensionable.hpp:94-149), their types known together (mpcx::HookSet).
//
// The same source compiled by hipcc for gfx950 runs the kernels on the GPU (tests/test_nlmpc_hooks_wg.py, the gpu tests).
//
//   run_hooks_wg <model> <hard> <max_iter> <form> [key=value ...] < instances
//     model: vanderpol (ph 10, ch 5, Ts 0.1) | vanderpol_terminal (the same with x(ph) = 0 and the cost on the outputs y = x) | ugv (ph 12, ch 4,
//            discrete, y = x) | chain9 (nine discrete integrators in a chain, ph 6, ch 3, a terminal equality, input rows);
//            form: wave (nlmpc_sqp, one wavefront per instance) | wg (workgroup form; waves per instance: HIPEMU_WAVES=1|2|4|8, default the plan's)
//     keys: lbu= ubu= (scalar input bounds on every block), repeat=N (N solves of the batch: same_bits says whether every one gave the first's bits)
//   stdin: one instance per line: x0[nx] u0[nu]
//   stdout: one JSON object per instance
// The controller's workspace is laid out as the library lays out a hook model's (engine::nlmpc_plan) with the workgroup form's hook buffers
// reserved (NlmpcDev::wg_hook_waves).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#if !defined(__HIPCC__)
// what the driver and mpcx/nlmpc_hooks.hpp's device-pointer path (ErasedHooks, not used here) name and the interpreter's runtime lacks (hipMalloc and hipFree it has): host memory
enum hipMemcpyKind { hipMemcpyHostToDevice = 1, hipMemcpyDeviceToHost = 2 };
inline hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind) { std::memcpy(d, s, n); return hipSuccess; }
inline hipError_t hipDeviceSynchronize() { return hipSuccess; }
#endif

#include "mpcx/nlmpc_hooks.hpp"
#include "mpcx/nlmpc_sqp_wg.hpp"

#if !defined(__HIPCC__)
namespace mpcx { namespace engine {
alignas(64) double smem[40960];
extern double lds_base[] __attribute__((alias("_ZN4mpcx6engine4smemE")));
} }
#endif

using namespace mpcx;

namespace sys {
// examples/vanderpol_ex.cpp:33-65
constexpr int VPH = 10, VCH = 5;
struct VdpState {
    __device__ void operator()(mpc::cvec<2> &dx, const mpc::cvec<2> &x, const mpc::cvec<1> &u, const unsigned int &) const
    {
        dx(0) = ((1.0 - (x(1) * x(1))) * x(0)) - x(1) + u(0);
        dx(1) = x(0);
    }
};
struct VdpObj {
    __device__ double operator()(const mpc::mat<VPH + 1, 2> &x, const mpc::mat<VPH + 1, 2> &, const mpc::mat<VPH + 1, 1> &u, const double &) const
    {
        return x.array().square().sum() + u.array().square().sum();
    }
};
struct VdpIneq {
    __device__ void operator()(mpc::cvec<VPH + 1> &in_con, const mpc::mat<VPH + 1, 2> &, const mpc::mat<VPH + 1, 2> &, const mpc::mat<VPH + 1, 1> &u,
                               const double &) const
    {
        for (int i = 0; i < VPH + 1; i++) in_con(i) = u(i, 0) - 0.5;
    }
};
// the same with the terminal equality x(ph) = 0 and the cost written on the outputs y = x
struct VdpOut {
    __device__ void operator()(mpc::cvec<2> &y, const mpc::cvec<2> &x, const mpc::cvec<1> &, const unsigned int &) const { y(0) = x(0); y(1) = x(1); }
};
struct VdpObjY {
    __device__ double operator()(const mpc::mat<VPH + 1, 2> &, const mpc::mat<VPH + 1, 2> &y, const mpc::mat<VPH + 1, 1> &u, const double &) const
    {
        return y.array().square().sum() + u.array().square().sum();
    }
};
struct VdpEq {
    __device__ void operator()(mpc::cvec<2> &eq_con, const mpc::mat<VPH + 1, 2> &x, const mpc::mat<VPH + 1, 1> &) const
    {
        eq_con(0) = x(VPH, 0); eq_con(1) = x(VPH, 1);
    }
};
// examples/ugv_ex.cpp:32-124 (the discrete double integrator, two obstacles, y = x)
constexpr int GPH = 12, GCH = 4;
constexpr double GTs = 0.1;
struct Obstacle { double px, py, radius; };
struct UgvState {
    __device__ void operator()(mpc::cvec<4> &dx, const mpc::cvec<4> &x, const mpc::cvec<2> &u, const unsigned int &) const
    {
        dx(0) = x(0) + GTs * x(2) + 0.5 * GTs * GTs * u(0); dx(1) = x(1) + GTs * x(3) + 0.5 * GTs * GTs * u(1);
        dx(2) = x(2) + GTs * u(0); dx(3) = x(3) + GTs * u(1);
    }
};
struct UgvOut {
    __device__ void operator()(mpc::cvec<4> &y, const mpc::cvec<4> &x, const mpc::cvec<2> &, const unsigned int &) const { y = x; }
};
struct UgvObj {
    __device__ double operator()(const mpc::mat<GPH + 1, 4> &x, const mpc::mat<GPH + 1, 4> &, const mpc::mat<GPH + 1, 2> &u, const double &e) const
    {
        mpc::cvec<2> v_pref; v_pref(0) = 0.7071067811865476; v_pref(1) = 0.7071067811865476;
        double cost = 0;
        for (int i = 0; i < GPH + 1; i++) {
            cost += 1e3 * (x.row(i).segment(2, 2).transpose() - v_pref).squaredNorm();
            cost += 1e-2 * u.row(i).squaredNorm();
        }
        cost += 1e-5 * e * e;
        return cost;
    }
};
struct UgvIneq {
    __device__ void operator()(mpc::cvec<2 * (GPH + 1)> &in_con, const mpc::mat<GPH + 1, 4> &x, const mpc::mat<GPH + 1, 4> &, const mpc::mat<GPH + 1, 2> &,
                               const double &) const
    {
        const Obstacle obs[2] = {{2.0, 1.0, 0.3}, {1.0, 1.0, 0.3}};
        int index = 0;
        for (int i = 0; i < GPH + 1; i++)
            for (int j = 0; j < 2; j++) {
                const double rx = x(i, 0) - obs[j].px, ry = x(i, 1) - obs[j].py;
                in_con(index++) = obs[j].radius - sqrt(rx * rx + ry * ry);
            }
    }
};
using Vdp = HookModel<2, 1, 2, VPH, VCH, VPH + 1, 0, HookSet<VdpState, VdpObj, VdpIneq>, 1, 0>;
using VdpTerminal = HookModel<2, 1, 2, VPH, VCH, VPH + 1, 2, HookSet<VdpState, VdpObjY, VdpIneq, VdpEq, VdpOut>, 1, 1>;
using Ugv = HookModel<4, 2, 4, GPH, GCH, 2 * (GPH + 1), 0, HookSet<UgvState, UgvObj, UgvIneq, NoHook, UgvOut>, 0, 1>;
// a wide state (NX > 8: every sub-problem row as long as the whole input part, the slack column included) with an equality: nine
// integrators in a chain driven at the first, the terminal first state pinned, |u| <= 1 as rows
constexpr int CPH = 6, CCH = 3;
struct ChainState {
    __device__ void operator()(mpc::cvec<9> &dx, const mpc::cvec<9> &x, const mpc::cvec<1> &u, const unsigned int &) const
    {
        dx(0) = x(0) + 0.1 * u(0);
        for (int i = 1; i < 9; i++) dx(i) = x(i) + 0.1 * x(i - 1);
    }
};
struct ChainObj {
    __device__ double operator()(const mpc::mat<CPH + 1, 9> &x, const mpc::mat<CPH + 1, 9> &, const mpc::mat<CPH + 1, 1> &u, const double &e) const
    {
        return x.array().square().sum() + 0.1 * u.array().square().sum() + 10.0 * e * e;
    }
};
struct ChainIneq {
    __device__ void operator()(mpc::cvec<2 * CPH> &in_con, const mpc::mat<CPH + 1, 9> &, const mpc::mat<CPH + 1, 9> &, const mpc::mat<CPH + 1, 1> &u,
                               const double &e) const
    {
        for (int i = 0; i < CPH; i++) { in_con(2 * i) = u(i, 0) - 1.0 - e; in_con(2 * i + 1) = -u(i, 0) - 1.0 - e; }
    }
};
struct ChainEq {
    __device__ void operator()(mpc::cvec<1> &eq_con, const mpc::mat<CPH + 1, 9> &x, const mpc::mat<CPH + 1, 1> &) const { eq_con(0) = x(CPH, 0); }
};
using Chain = HookModel<9, 1, 9, CPH, CCH, 2 * CPH, 1, HookSet<ChainState, ChainObj, ChainIneq, ChainEq>, 0, 0>;
}  // namespace sys

template <class T> static T *to_dev(const std::vector<T> &h)
{
    void *p = nullptr;
    if (hipMalloc(&p, h.size() * sizeof(T) + 16) != hipSuccess) { fprintf(stderr, "hipMalloc failed\n"); exit(6); }
    if (!h.empty()) (void)hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    return static_cast<T *>(p);
}
template <class T> static std::vector<T> from_dev(const T *d, size_t n)
{
    std::vector<T> h(n);
    if (hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) { fprintf(stderr, "hipMemcpy failed\n"); exit(6); }
    return h;
}

template <class Mdl, class Hooks>
static int run(int argc, char **argv, double Ts)
{
    const int hard = atoi(argv[2]), max_iter = atoi(argv[3]);
    const std::string form = argv[4];
    double lbu = -INFINITY, ubu = INFINITY;
    int repeat = 1;
    for (int a = 5; a < argc; ++a) {
        std::string kv = argv[a];
        const size_t eq = kv.find('=');
        const std::string k = kv.substr(0, eq), v = kv.substr(eq + 1);
        if (k == "lbu") lbu = atof(v.c_str()); else if (k == "ubu") ubu = atof(v.c_str()); else if (k == "repeat") repeat = atoi(v.c_str());
        else { fprintf(stderr, "unknown key %s\n", k.c_str()); return 2; }
    }
    constexpr int NX = Mdl::NX, NU = Mdl::NU, NYA = Mdl::NY > 0 ? Mdl::NY : 1, ph = Mdl::PH, ch = Mdl::CH;
    // the controller as the library sets up a hook model (mpcx_nlmpc_create_hooked): the closures are the parameters
    const Hooks hooks{};
    std::vector<unsigned char> hb(sizeof(Hooks));
    std::memcpy(hb.data(), &hooks, sizeof(Hooks));
    NlmpcDev M{};
    M.nx = NX; M.nu = NU; M.ny = Mdl::NY; M.ph = ph; M.ch = ch; M.nineq = Mdl::NI; M.nue = Mdl::NE; M.Ts = Ts;
    M.continuous = Ts > 0.0 ? 1 : 0; M.has_output = Mdl::HAS_OUTPUT ? 1 : 0; M.vector_hooks = 1;
    M.wg_hook_waves = form == "wg" ? (engine::kWgEightWaves<Mdl> ? 8 : 4) : 0;
    M.params = reinterpret_cast<const double *>(to_dev(hb));
    M.su = to_dev(std::vector<double>(NU, 1.0)); M.ss = to_dev(std::vector<double>(NX, 1.0)); M.iss = to_dev(std::vector<double>(NX, 1.0)); M.scaled = 0;
    M.nbnd = 0;
    engine::nlmpc_plan(M);
    const int nz = M.nz, nxs = ph * NX;
    std::vector<double> lb(nz, -INFINITY), ub(nz, INFINITY);
    for (int k = 0; k < ch * NU; ++k) { lb[nxs + k] = lbu; ub[nxs + k] = ubu; }
    std::vector<int> bidx; std::vector<double> bsign, bval;
    for (int k = 0; k < nz - 1; ++k) {
        if (ub[k] < 1e30) { bidx.push_back(k); bsign.push_back(1.0); bval.push_back(ub[k]); }
        if (lb[k] > -1e30) { bidx.push_back(k); bsign.push_back(-1.0); bval.push_back(lb[k]); }
    }
    bidx.push_back(0); bsign.push_back(0); bval.push_back(0);
    M.zlb = to_dev(lb); M.zub = to_dev(ub); M.nbnd = (int)bidx.size() - 1; M.nbnd_state = 0;
    M.bnd_idx = to_dev(bidx); M.bnd_sign = to_dev(bsign); M.bnd_val = to_dev(bval);
    engine::nlmpc_plan(M);
    const int mt = M.nineq + M.nue + M.nbnd;
    engine::WgPlan P{};
    if (form == "wg") {
        const int waves = getenv("HIPEMU_WAVES") ? atoi(getenv("HIPEMU_WAVES")) : 0;
        if (engine::wg_plan<Mdl>(M, hard, waves, 0, P) != 0) { fprintf(stderr, "the workgroup form does not take this shape\n"); return 3; }
        if (getenv("HIPEMU_VERBOSE")) fprintf(stderr, "wg plan: waves %d, lds %d doubles, kw %d, nd %d, nsx %d, ws %d of %d doubles, curv0 %d\n", P.waves, P.lds_total, P.kw, P.nd, P.nsx, P.ws_total, M.ws.scal, P.curv0);
    }
    std::vector<double> X0, U0;
    for (;;) {
        std::vector<double> row(NX + NU);
        bool ok = true;
        for (double &v : row) ok = ok && scanf("%lf", &v) == 1;
        if (!ok) break;
        X0.insert(X0.end(), row.begin(), row.begin() + NX); U0.insert(U0.end(), row.begin() + NX, row.end());
    }
    const int B = (int)(X0.size() / NX);
    const size_t ws_total = M.ws.total;
#if !defined(__HIPCC__)
    // (workspace and LDS start as NaNs: a kernel that reads what it has not written shows it)
    std::fill(engine::smem, engine::smem + 40960, std::nan(""));
#endif
    const size_t nS = (size_t)B * (ph + 1) * NX, nU = (size_t)B * (ph + 1) * NU, nY = (size_t)B * (ph + 1) * NYA, nM = (size_t)B * (mt > 0 ? mt : 1);
    double *ws = to_dev(std::vector<double>((size_t)B * ws_total, std::nan("")));
    double *cmd = to_dev(std::vector<double>((size_t)B * NU)), *cost = to_dev(std::vector<double>(B)), *zout = to_dev(std::vector<double>((size_t)B * nz));
    double *sx = to_dev(std::vector<double>(nS)), *su = to_dev(std::vector<double>(nU)), *sy = to_dev(std::vector<double>(nY)), *mu = to_dev(std::vector<double>(nM));
    int *status = to_dev(std::vector<int>(B)), *sstat = to_dev(std::vector<int>(B)), *feas = to_dev(std::vector<int>(B)), *iters = to_dev(std::vector<int>(B));
    NlmpcSolveDev S{};
    S.batch = B; S.x0 = to_dev(X0); S.u0 = to_dev(U0); S.z_warm = nullptr; S.ws = ws; S.max_iter = max_iter; S.hard = hard;
    S.keep_curvature = 0; S.tol_step = 1e-6; S.tol_con = 1e-8; S.ieq_tol = 1e-10; S.eq_tol = 1e-10;
    S.ftol_rel = S.ftol_abs = S.xtol_rel = S.xtol_abs = -1.0;
    S.cmd = cmd; S.cost = cost; S.z_out = zout; S.status = status; S.solver_status = sstat;
    S.is_feasible = feas; S.iterations = iters; S.seq_state = sx; S.seq_input = su; S.seq_output = sy; S.mu_out = mu;
    std::vector<double> hc, hcost, hz, hsx, hsy;
    std::vector<int> hst, hss, hfe, hit;
    bool same = true;
    for (int r = 0; r < repeat; ++r) {
        const int rc = form == "wg" ? engine::launch_solve_wg<Mdl>(&M, &S, &P, nullptr) : engine::launch_solve<Mdl>(nullptr, &M, &S, nullptr);
        if (rc != 0 || hipDeviceSynchronize() != hipSuccess) { fprintf(stderr, "launch failed: %d\n", rc); return 4; }
        auto c = from_dev(cmd, (size_t)B * NU), co = from_dev(cost, B), z = from_dev(zout, (size_t)B * nz);
        auto st = from_dev(status, B), ss = from_dev(sstat, B), it = from_dev(iters, B);
        if (r == 0) {
            hc = c; hcost = co; hz = z; hst = st; hss = ss; hit = it;
            hsx = from_dev(sx, nS); hsy = from_dev(sy, nY); hfe = from_dev(feas, B);
        } else {
            same = same && !std::memcmp(c.data(), hc.data(), c.size() * sizeof(double)) && !std::memcmp(co.data(), hcost.data(), co.size() * sizeof(double)) &&
                   !std::memcmp(z.data(), hz.data(), z.size() * sizeof(double)) && st == hst && ss == hss && it == hit;
        }
    }
    for (int b = 0; b < B; ++b) {
        printf("{\"b\": %d, \"status\": %d, \"solver_status\": %d, \"feasible\": %d, \"iterations\": %d, \"same_bits\": %d, \"cost\": %.17g, \"cmd\": [", b, hst[b], hss[b],
               hfe[b], hit[b], same ? 1 : 0, std::isfinite(hcost[b]) ? hcost[b] : 1e308);
        for (int j = 0; j < NU; ++j) printf("%s%.17g", j ? ", " : "", hc[b * NU + j]);
        printf("], \"z\": [");
        for (int k = 0; k < nz; ++k) printf("%s%.17g", k ? ", " : "", hz[(size_t)b * nz + k]);
        printf("], \"seq_state\": [");
        for (int k = 0; k < (ph + 1) * NX; ++k) printf("%s%.17g", k ? ", " : "", hsx[(size_t)b * (ph + 1) * NX + k]);
        printf("], \"seq_output\": [");
        for (int k = 0; k < (ph + 1) * Mdl::NY; ++k) printf("%s%.17g", k ? ", " : "", hsy[(size_t)b * (ph + 1) * NYA + k]);
        printf("]}\n");
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 5) { fprintf(stderr, "usage: run_hooks_wg model hard max_iter form [key=value ...]\n"); return 2; }
    const std::string m = argv[1];
    if (m == "vanderpol") return run<sys::Vdp, HookSet<sys::VdpState, sys::VdpObj, sys::VdpIneq>>(argc, argv, 0.1);
    if (m == "vanderpol_terminal") return run<sys::VdpTerminal, HookSet<sys::VdpState, sys::VdpObjY, sys::VdpIneq, sys::VdpEq, sys::VdpOut>>(argc, argv, 0.1);
    if (m == "ugv") return run<sys::Ugv, HookSet<sys::UgvState, sys::UgvObj, sys::UgvIneq, NoHook, sys::UgvOut>>(argc, argv, 0.0);
    if (m == "chain9") return run<sys::Chain, HookSet<sys::ChainState, sys::ChainObj, sys::ChainIneq, sys::ChainEq>>(argc, argv, 0.0);
    fprintf(stderr, "unknown model %s\n", m.c_str());
    return 2;
}
