// ctk_host.h — host helpers that the two host translation units share: ctk_api.hip (the single handle) defines them, ctk_batch.hip (the
// batch families) uses them.  Private to the library: hidden visibility, so none of them is an exported symbol.
#pragma once
#include <cmath>
#include <string>
#include <vector>

#include "ctk_launch.h"
#include "ctk_env.h"      // EnvInfo

#pragma GCC visibility push(hidden)
namespace ctk_host {

// the text of a refused creation, of a handle or of a batch of any family: ONE thread-local, read by every *_last_error(NULL)
extern thread_local std::string g_create_error;

const EnvInfo* env_info(int env);   // NULL: not an environment of this library
int num_inducing_points(int H, int p);
std::vector<InterpEntry> build_interp_table(int H, int p, int P);
MppiK mppi_constants(const ctk_config& c);
void default_params(int env, float* p);
std::vector<float> permute_mlp_weights(const float* raw, int S = CTK_S, int C = CTK_C);
size_t weight_count(int predictor, int S, int C, int hid = 32);
size_t shaped_weight_count(int predictor, int S, int C, int h1, int h2);
void embed_mlp_rows(const float* w, int S, int I, int h1, int h2, int W, float* full);
int check_config(const char* who, const ctk_config* cfg, const EnvInfo** einfo_out);
int probe_device(const char* who, int device, hipDeviceProp_t* prop);

// Adam's bias corrections {1 - beta_1^t, 1 - beta_2^t}, t = 1 .. 32768, in double, rounded to fp32 (optimizer_rpgd.py:73-74); beyond the
// table both are exactly 1.0f in fp32
inline std::vector<float> adam_bias_corrections(float beta_1, float beta_2) {
    std::vector<float> bc((size_t)2 * 32768);
    for (size_t tt = 1; 2 * tt <= bc.size(); ++tt) {
        bc[2 * (tt - 1)] = (float)(1.0 - std::pow((double)beta_1, (double)tt));
        bc[2 * (tt - 1) + 1] = (float)(1.0 - std::pow((double)beta_2, (double)tt));
    }
    return bc;
}

}  // namespace ctk_host
#pragma GCC visibility pop
